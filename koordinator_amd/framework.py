"""Host-side mirror of the reference's plugin surface for the accelerated path.

The reference's Go host (koord-scheduler) cannot run here (no Go toolchain); this module is the host layer
above the C ABI with the reference's names and argument meanings, so tests read like the reference's own:

* ``LoadAwareSchedulingArgs`` — pkg/scheduler/apis/config/types.go:30-76, defaults v1beta2/defaults.go:76-99.
* ``NodeResourcesFitArgs`` — upstream NodeResourcesFitArgs, scoringStrategy LeastAllocated.
* ``Profile`` — the score plugin set + weights of a KubeSchedulerConfiguration profile
  (config/manager/scheduler-config.yaml:82-91).
* ``make_node / make_node_metric / make_pod`` — what the Go shim decodes from corev1.Node, NodeMetric and
  corev1.Pod (allocatable, raw-allocatable and custom-usage-threshold annotations, PodRequestsAndLimits,
  GetPodPriorityClassWithDefault).
* ``Scheduler`` — SchedulePod for a FIFO queue (frameworkext SchedulePod interception,
  framework_extender_factory.go:136-185), RunFilterPlugins / RunScorePlugins for one pod
  (framework_extender.go:204-258), Reserve/Unreserve (kg_pods_add / kg_pods_remove).
Status codes mirror framework.Code: Success, Unschedulable.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from . import abi
from .engine import Engine
from .quantity import resource_value

SUCCESS, UNSCHEDULABLE = "Success", "Unschedulable"
NODE_RESOURCES_FIT, LOAD_AWARE, NODE_NUMA_RESOURCE = "NodeResourcesFit", "LoadAwareScheduling", "NodeNUMAResource"
DEVICE_SHARE = "DeviceShare"
RESERVATION = "Reservation"
# upstream default plugins a stock profile keeps (k8s v1.24.15 v1beta2 defaults: Score weight 1 each)
TAINT_TOLERATION, NODE_AFFINITY = "TaintToleration", "NodeAffinity"
BALANCED_ALLOCATION = "NodeResourcesBalancedAllocation"
IMAGE_LOCALITY = "ImageLocality"
# (ABI 12) hostname-keyed PodTopologySpread (default weight 2) and InterPodAffinity (default weight 1)
POD_TOPOLOGY_SPREAD, INTER_POD_AFFINITY = "PodTopologySpread", "InterPodAffinity"

# (ABI 18) kg_topn_row.plugin[KG_PL_*] -> the plugin's name (the column headers of --debug-scores)
PLUGIN_COLUMNS = {
    abi.PL_FIT: NODE_RESOURCES_FIT, abi.PL_LOADAWARE: LOAD_AWARE, abi.PL_NUMA: NODE_NUMA_RESOURCE,
    abi.PL_DEVICESHARE: DEVICE_SHARE, abi.PL_RESERVATION: RESERVATION, abi.PL_TAINT: TAINT_TOLERATION,
    abi.PL_NODE_AFFINITY: NODE_AFFINITY, abi.PL_BALANCED: BALANCED_ALLOCATION, abi.PL_IMAGE_LOCALITY: IMAGE_LOCALITY,
}
# the kg_config field that enables each column's plugin at Score
_PLUGIN_SCORE_FIELD = {
    abi.PL_FIT: "fit_score", abi.PL_LOADAWARE: "la_score", abi.PL_NUMA: "numa_score", abi.PL_DEVICESHARE: "ds_score",
    abi.PL_RESERVATION: "reservation_score", abi.PL_TAINT: "taint_score", abi.PL_NODE_AFFINITY: "affinity_score",
    abi.PL_BALANCED: "balanced_score", abi.PL_IMAGE_LOCALITY: "image_score",
}

# (kg_pods_diagnose) KG_REJECT_* bit -> the reason string FitError.Error() counts.  NodeResourcesFit's are upstream's
# texts (noderesources/fit.go).  Where the reference's message carries a parameter the engine's bit does not (LoadAware's
# "node(s) %s usage exceed threshold", the untolerated taint's key and value, the insufficient scalar resource's name,
# NodeNUMAResource's / DeviceShare's / Reservation's several causes) there is one fixed class string per bit: these are
# the engine's reason classes, not byte-equal to the Go messages.
REASON_STRINGS = {
    abi.REJECT_FIT_PODS: "Too many pods",
    abi.REJECT_FIT_CPU: "Insufficient cpu",
    abi.REJECT_FIT_MEMORY: "Insufficient memory",
    abi.REJECT_FIT_OTHER: "Insufficient ephemeral-storage or scalar resource",
    abi.REJECT_LOADAWARE: "node(s) usage exceed threshold",
    abi.REJECT_NUMA: "node(s) NUMA topology or cpuset unsatisfied",
    abi.REJECT_DEVICE: "Insufficient devices",
    abi.REJECT_RESERVATION: "node(s) no reservation satisfies the pod or reservation policy conflict",
    abi.REJECT_TAINT: "node(s) had untolerated taint",
    abi.REJECT_NODE_AFFINITY: "node(s) didn't match Pod's node affinity/selector",
}


@dataclass(frozen=True)
class FitError:
    """framework.FitError of one pod as kg_pods_diagnose counts it: NumAllNodes, the feasible nodes, the NodeToStatusMap
    reasons histogram and Diagnosis.UnschedulablePlugins (the plugins some node's status comes from).  `reasons` maps
    REASON_STRINGS texts to node counts: the engine's reason classes, not byte-equal to the Go messages where those
    carry a parameter.  message() follows upstream v1.24 FitError.Error(); upstream is not vendored in the reference
    tree, so its exact text is parity-unpinned like the other upstream pieces."""
    num_all_nodes: int
    feasible_nodes: int
    reasons: dict
    unschedulable_plugins: frozenset

    @classmethod
    def from_diag(cls, diag) -> "FitError":
        """From one abi.FIT_DIAG_DTYPE record (or a mapping with the same fields)."""
        reasons = {text: int(diag["reason_nodes"][bit.bit_length() - 1]) for bit, text in REASON_STRINGS.items()
                   if int(diag["reason_nodes"][bit.bit_length() - 1]) > 0}
        plugins = frozenset(name for k, name in PLUGIN_COLUMNS.items() if int(diag["plugin_nodes"][k]) > 0)
        return cls(int(diag["num_all_nodes"]), int(diag["feasible"]), reasons, plugins)

    def message(self) -> str:
        """`0/N nodes are available: ` + the "count reason" strings sorted as strings, joined by ", " + `.`
        (scheduler/framework/types.go FitError.Error(), v1.24); reasons with a zero count are left out."""
        parts = sorted(f"{int(v)} {k}" for k, v in self.reasons.items() if int(v) > 0)
        return f"0/{self.num_all_nodes} nodes are available: " + ", ".join(parts) + "."


def render_debug_table(rows, plugin_columns, pod_ref: str, node_names) -> str:
    """The Markdown table frameworkext's debugScores renders (frameworkext/debug.go:83-107, go-pretty RenderMarkdown):
    header `#`, `Pod`, `Node`, `Score`, then the plugin names sorted as strings; one line per row, in the order given
    (kg_debug_topn ranks them).  rows: kg_topn_row records or plain mappings with "node_idx", "total" and "plugin"
    (indexable by column); plugin_columns: {column: plugin name} of the columns to print; node_names: node index ->
    name.  Text columns are left-aligned (`---`), numbers right-aligned (`---:`), as go-pretty writes them."""
    cols = sorted(plugin_columns.items(), key=lambda kv: kv[1])
    lines = ["| " + " | ".join(["#", "Pod", "Node", "Score"] + [name for _, name in cols]) + " |",
             "|" + " --- |" * 3 + " ---:|" * (1 + len(cols))]
    for i, r in enumerate(rows):
        cells = [str(i), pod_ref, str(node_names[int(r["node_idx"])]), str(int(r["total"]))]
        cells += [str(int(r["plugin"][c])) for c, _ in cols]
        lines.append("| " + " | ".join(cells) + " |")
    return "\n".join(lines)


def _slots(d: dict | None, absent=0) -> np.ndarray:
    out = np.full(abi.RES_MAX, absent, dtype=np.int64)
    for k, v in (d or {}).items():
        out[abi.RESOURCE_SLOTS[k]] = int(v)
    return out


@dataclass
class LoadAwareSchedulingArgs:
    filter_expired_node_metrics: bool = True
    node_metric_expiration_seconds: int | None = 180
    resource_weights: dict = field(default_factory=lambda: {"cpu": 1, "memory": 1})
    usage_thresholds: dict = field(default_factory=lambda: {"cpu": 65, "memory": 95})
    prod_usage_thresholds: dict = field(default_factory=dict)
    score_according_prod_usage: bool = False
    estimated_scaling_factors: dict = field(default_factory=lambda: {"cpu": 85, "memory": 70})
    # Aggregated (config/types.go:56-76): usage_thresholds / usage_type ("p95", ...) / usage_duration_s for Filter,
    # score_type / score_duration_s for Score; duration 0 = the longest period recorded
    aggregated: dict | None = None


@dataclass
class NodeResourcesFitArgs:
    """Upstream NodeResourcesFitArgs.ScoringStrategy: Type (LeastAllocated / MostAllocated / RequestedToCapacityRatio),
    Resources weights and, for RequestedToCapacityRatio, RequestedToCapacityRatio.Shape as (utilization, score) pairs.
    kg_config has no room for a shape: build_config leaves the strategy word 0 for it, and the shape goes to the engine
    right after create — Scheduler(config, capacity, fit=args) / Engine(..., fit_shape=args.shape) do that."""
    scoring_resources: dict = field(default_factory=lambda: {"cpu": 1, "memory": 1})
    scoring_strategy: str = "LeastAllocated"
    shape: list | None = None


REQUESTED_TO_CAPACITY_RATIO = "RequestedToCapacityRatio"


def validate_fit_shape(points) -> np.ndarray:
    """The shape as an array of kg_shape_point, after kg_fit_shape_set's checks: 1 to 101 points, utilization strictly
    increasing within [0, 100], score within [0, 10].  ValueError otherwise."""
    pts = [(int(u), int(s)) for u, s in points]
    if not 1 <= len(pts) <= abi.FIT_SHAPE_MAX_POINTS:
        raise ValueError(f"RequestedToCapacityRatio shape: {len(pts)} points (1 to {abi.FIT_SHAPE_MAX_POINTS})")
    for i, (u, sc) in enumerate(pts):
        if not 0 <= u <= 100:
            raise ValueError(f"RequestedToCapacityRatio shape point {i}: utilization {u} outside [0, 100]")
        if i and u <= pts[i - 1][0]:
            raise ValueError(f"RequestedToCapacityRatio shape point {i}: utilization must be strictly increasing")
        if not 0 <= sc <= 10:
            raise ValueError(f"RequestedToCapacityRatio shape point {i}: score {sc} outside [0, 10]")
    return np.array(pts, dtype=abi.SHAPE_POINT_DTYPE)


@dataclass
class NodeNUMAResourceArgs:
    """pkg/scheduler/apis/config/types.go NodeNUMAResourceArgs; defaults v1beta2/defaults.go:101-137."""
    default_cpu_bind_policy: str = "FullPCPUs"
    scoring_strategy: str = "LeastAllocated"
    scoring_resources: dict = field(default_factory=lambda: {"cpu": 1, "memory": 1})
    numa_scoring_strategy: str = "LeastAllocated"
    numa_scoring_resources: dict = field(default_factory=lambda: {"cpu": 1, "memory": 1})


@dataclass
class DeviceShareArgs:
    """pkg/scheduler/apis/config/types.go DeviceShareArgs; defaults v1beta2/defaults.go:187-208 (LeastAllocated on
    gpu-memory-ratio / rdma / fpga, weight 1 — rdma and fpga weights only touch RDMA / FPGA devices)."""
    scoring_strategy: str = "LeastAllocated"
    scoring_resources: dict = field(default_factory=lambda: {"koordinator.sh/gpu-memory-ratio": 1,
                                                             "koordinator.sh/rdma": 1, "koordinator.sh/fpga": 1})


@dataclass
class Profile:
    filter: tuple = (NODE_RESOURCES_FIT, LOAD_AWARE)
    score: dict = field(default_factory=lambda: {NODE_RESOURCES_FIT: 1, LOAD_AWARE: 1})


def build_config(la: LoadAwareSchedulingArgs | None = None, fit: NodeResourcesFitArgs | None = None,
                 profile: Profile | None = None, batch_pods: int = 32, pods_per_wave: int = 8,
                 device_id: int = -1, numa: NodeNUMAResourceArgs | None = None,
                 deviceshare: DeviceShareArgs | None = None, pipeline_depth: int = 0,
                 balanced_resources: tuple = ("cpu", "memory"), hard_pod_affinity_weight: int = 1,
                 multi_rank: str = "auto") -> np.ndarray:
    """kg_config of a profile.  multi_rank (ABI 15): "shard" / "replica" / "auto" — how an engine of several ranks
    splits the work (kg_config.multi_rank_mode).  balanced_resources: NodeResourcesBalancedAllocationArgs.resources (v1beta2 default
    cpu + memory, weight 1 each; the weights do not enter the two-resource std).  hard_pod_affinity_weight:
    InterPodAffinityArgs.HardPodAffinityWeight (v1beta2 default 1)."""
    la = la or LoadAwareSchedulingArgs()
    fit = fit or NodeResourcesFitArgs()
    profile = profile or Profile()
    numa = numa or NodeNUMAResourceArgs()
    ds = deviceshare or DeviceShareArgs()
    c = np.zeros(1, dtype=abi.CONFIG_DTYPE)
    r = c[0]
    r["abi_version"] = abi.ABI_VERSION
    r["la_filter_expired_node_metrics"] = int(la.filter_expired_node_metrics)
    r["la_node_metric_expiration_seconds"] = -1 if la.node_metric_expiration_seconds is None else la.node_metric_expiration_seconds
    r["la_resource_weights"] = _slots(la.resource_weights)
    r["la_usage_thresholds"] = _slots(la.usage_thresholds)
    r["la_prod_usage_thresholds"] = _slots(la.prod_usage_thresholds)
    r["la_estimated_scaling_factors"] = _slots(la.estimated_scaling_factors)
    r["la_score_according_prod_usage"] = int(la.score_according_prod_usage)
    agg = la.aggregated or {}
    r["la_agg_usage_thresholds"] = _slots(agg.get("usage_thresholds"))
    r["la_agg_usage_type"] = abi.AGG_TYPES[agg.get("usage_type", "")]
    r["la_agg_usage_duration_ns"] = int(agg.get("usage_duration_s", 0) * 10**9)
    r["la_agg_score_type"] = abi.AGG_TYPES[agg.get("score_type", "")]
    r["la_agg_score_duration_ns"] = int(agg.get("score_duration_s", 0) * 10**9)
    r["fit_resource_weights"] = _slots(fit.scoring_resources)
    if fit.scoring_strategy == REQUESTED_TO_CAPACITY_RATIO and fit.shape is not None:
        # the shape travels by kg_fit_shape_set after create (Scheduler(..., fit=fit)); the config word stays 0
        validate_fit_shape(fit.shape)
        r["fit_scoring_strategy"] = 0
    elif fit.scoring_strategy not in abi.STRATEGY:
        # RequestedToCapacityRatio without its shape, or an unknown type
        raise ValueError(f"NodeResourcesFitArgs.ScoringStrategy.Type {fit.scoring_strategy!r}: the engine scores "
                         f"{' / '.join(abi.STRATEGY)}, and {REQUESTED_TO_CAPACITY_RATIO} given its shape")
    else:
        r["fit_scoring_strategy"] = abi.STRATEGY[fit.scoring_strategy]
    r["fit_filter"] = int(NODE_RESOURCES_FIT in profile.filter)
    r["la_filter"] = int(LOAD_AWARE in profile.filter)
    r["fit_score"] = int(NODE_RESOURCES_FIT in profile.score)
    r["la_score"] = int(LOAD_AWARE in profile.score)
    r["weight_fit"] = int(profile.score.get(NODE_RESOURCES_FIT, 0))
    r["weight_loadaware"] = int(profile.score.get(LOAD_AWARE, 0))
    r["batch_pods"] = batch_pods
    r["pods_per_wave"] = pods_per_wave
    r["device_id"] = device_id
    r["pipeline_depth"] = pipeline_depth
    r["numa_filter"] = int(NODE_NUMA_RESOURCE in profile.filter)
    r["numa_score"] = int(NODE_NUMA_RESOURCE in profile.score)
    r["weight_numa"] = int(profile.score.get(NODE_NUMA_RESOURCE, 0))
    r["numa_default_cpu_bind_policy"] = abi.BIND[numa.default_cpu_bind_policy]
    r["numa_scoring_strategy"] = abi.STRATEGY[numa.scoring_strategy]
    r["numa_scoring_weights"] = [numa.scoring_resources.get("cpu", 0), numa.scoring_resources.get("memory", 0)]
    r["numa_numa_scoring_strategy"] = abi.STRATEGY[numa.numa_scoring_strategy]
    r["numa_numa_scoring_weights"] = [numa.numa_scoring_resources.get("cpu", 0),
                                      numa.numa_scoring_resources.get("memory", 0)]
    r["ds_filter"] = int(DEVICE_SHARE in profile.filter)
    r["ds_score"] = int(DEVICE_SHARE in profile.score)
    r["weight_deviceshare"] = int(profile.score.get(DEVICE_SHARE, 0))
    r["reservation_filter"] = int(RESERVATION in profile.filter)
    r["reservation_score"] = int(RESERVATION in profile.score)
    r["weight_reservation"] = int(profile.score.get(RESERVATION, 0))
    r["taint_filter"] = int(TAINT_TOLERATION in profile.filter)
    r["taint_score"] = int(TAINT_TOLERATION in profile.score)
    r["weight_taint"] = int(profile.score.get(TAINT_TOLERATION, 0))
    r["affinity_filter"] = int(NODE_AFFINITY in profile.filter)
    r["affinity_score"] = int(NODE_AFFINITY in profile.score)
    r["weight_affinity"] = int(profile.score.get(NODE_AFFINITY, 0))
    r["balanced_score"] = int(BALANCED_ALLOCATION in profile.score)
    r["weight_balanced"] = int(profile.score.get(BALANCED_ALLOCATION, 0))
    r["balanced_resources"] = sum({"cpu": 1, "memory": 2}.get(k, 1 << 8) for k in balanced_resources)
    r["image_score"] = int(IMAGE_LOCALITY in profile.score)
    r["weight_image"] = int(profile.score.get(IMAGE_LOCALITY, 0))
    r["spread_filter"] = int(POD_TOPOLOGY_SPREAD in profile.filter)
    r["spread_score"] = int(POD_TOPOLOGY_SPREAD in profile.score)
    r["weight_spread"] = int(profile.score.get(POD_TOPOLOGY_SPREAD, 0))
    r["interpod_filter"] = int(INTER_POD_AFFINITY in profile.filter)
    r["interpod_score"] = int(INTER_POD_AFFINITY in profile.score)
    r["weight_interpod"] = int(profile.score.get(INTER_POD_AFFINITY, 0))
    r["hard_pod_affinity_weight"] = hard_pod_affinity_weight
    r["multi_rank_mode"] = abi.MULTI_RANK[multi_rank]
    r["ds_scoring_strategy"] = abi.STRATEGY[ds.scoring_strategy]
    r["ds_scoring_weights"] = [ds.scoring_resources.get("koordinator.sh/gpu-core", 0),
                               ds.scoring_resources.get("koordinator.sh/gpu-memory", 0),
                               ds.scoring_resources.get("koordinator.sh/gpu-memory-ratio", 0)]
    r["ds_scoring_weights_x"] = [ds.scoring_resources.get("koordinator.sh/rdma", 0),
                                 ds.scoring_resources.get("koordinator.sh/fpga", 0)]
    return c


def _values(resources: dict | None) -> np.ndarray:
    out = np.zeros(abi.RES_MAX, dtype=np.int64)
    for k, v in (resources or {}).items():
        out[abi.RESOURCE_SLOTS[k]] = resource_value(k, v)
    return out


def make_node(allocatable: dict, allowed_pods: int = 110, raw_allocatable: dict | None = None,
              custom_usage_thresholds: dict | None = None, custom_prod_usage_thresholds: dict | None = None,
              valid: bool = True, custom_aggregated: dict | None = None) -> np.ndarray:
    """custom_aggregated = the annotation's AggregatedUsage {usage_thresholds, usage_type, usage_duration_s}."""
    n = np.zeros(1, dtype=abi.NODE_DTYPE)
    r = n[0]
    r["allocatable"] = _values(allocatable)
    r["allowed_pods"] = allowed_pods
    flags = abi.NODE_VALID if valid else 0
    if raw_allocatable:
        flags |= abi.NODE_HAS_RAW_ALLOCATABLE
        r["raw_allocatable"] = _values(raw_allocatable)
        pres = np.zeros(abi.RES_MAX, dtype=np.int64)
        for k in raw_allocatable:
            pres[abi.RESOURCE_SLOTS[k]] = 1
        r["raw_allocatable_present"] = pres
    r["custom_usage_thresholds"] = _slots(custom_usage_thresholds, absent=-1)
    r["custom_prod_usage_thresholds"] = _slots(custom_prod_usage_thresholds, absent=-1)
    ca = custom_aggregated or {}
    r["custom_agg_thresholds"] = _slots(ca.get("usage_thresholds"), absent=-1)
    r["custom_agg_type"] = abi.AGG_TYPES[ca.get("usage_type", "")]
    r["custom_agg_duration_ns"] = int(ca.get("usage_duration_s", 0) * 10**9)
    if custom_usage_thresholds or custom_prod_usage_thresholds or custom_aggregated:
        flags |= abi.NODE_HAS_CUSTOM_THRESHOLDS
    r["flags"] = flags
    return n


def make_node_metric(present: bool = True, update_time_ns: int | None = 0, node_usage: dict | None = None,
                     prod_pods_usage: dict | None = None, pods_metric_count: int = 0,
                     aggregated: list | None = None, report_interval_ns: int = 0) -> np.ndarray:
    """NodeMetric status summary; node_usage=None means Status.NodeMetric == nil.  aggregated = the
    AggregatedNodeUsages [{"duration_s": .., "p95": {"cpu": .., "memory": ..}, ...}]."""
    m = np.zeros(1, dtype=abi.METRIC_DTYPE)
    r = m[0]
    r["present"] = int(present)
    r["has_update_time"] = int(update_time_ns is not None)
    r["update_time_unix_nano"] = update_time_ns or 0
    if node_usage is not None:
        r["has_node_metric"] = 1
        r["node_usage"] = _values(node_usage)
        pres = np.zeros(abi.RES_MAX, dtype=np.int64)
        for k in node_usage:
            pres[abi.RESOURCE_SLOTS[k]] = 1
        r["node_usage_present"] = pres
    r["pods_metric_count"] = pods_metric_count
    r["report_interval_ns"] = report_interval_ns  # CollectPolicy.ReportIntervalSeconds; 0 = the 60 s default
    r["prod_pods_usage"] = _values(prod_pods_usage)
    aggs = aggregated or []
    if len(aggs) > 4:
        raise ValueError("at most 4 AggregatedNodeUsages")
    r["agg_count"] = len(aggs)
    for i, a in enumerate(aggs):
        r["agg_duration_ns"][i] = int(a.get("duration_s", 0) * 10**9)
        for name, t in abi.AGG_TYPES.items():
            if t == 0 or name not in a:
                continue
            for k, v in a[name].items():
                slot = abi.RESOURCE_SLOTS[k]
                if slot < 2:
                    r["agg_usage"][i, t - 1, slot] = resource_value(k, v)
                    r["agg_present"][i, t - 1] |= 1 << slot
    return m


def make_node_numa(sockets: int = 0, nodes_per_socket: int = 1, cores_per_node: int = 0, cpus_per_core: int = 2,
                   numa_policy: str = "", node_cpu_bind_policy: str = "", numa_allocate_strategy: str | None = None,
                   numa_resources: list | None = None, reserved_cpus=(), allocated_cpus=(),
                   numa_allocated: dict | None = None, cpu_amplification_ratio: float = 0.0,
                   exclusive_pcpu_cpus=(), exclusive_numa_cpus=()) -> np.ndarray:
    """NodeNUMAResource view of a node: the NodeResourceTopology's CPU topology (buildCPUTopology numbering),
    policies and zones, and the NodeAllocation of already-bound pods. numa_resources = [{"cpu": .., "memory": ..}]
    per NUMA zone; numa_allocated = {zone: {"cpu": .., "memory": ..}}; cpu_amplification_ratio = the node's
    node.koordinator.sh/resource-amplification-ratio cpu (≤ 1 none; zone cpu is given amplified);
    exclusive_{pcpu,numa}_cpus = the allocated cpus whose holder's CPUExclusivePolicy is PCPULevel / NUMANodeLevel."""
    n = np.zeros(1, dtype=abi.NODE_NUMA_DTYPE)
    r = n[0]
    r["has_topology"] = int(sockets > 0)
    r["sockets"], r["nodes_per_socket"], r["cores_per_node"], r["cpus_per_core"] = (
        sockets, nodes_per_socket, cores_per_node, cpus_per_core)
    r["numa_policy"] = abi.NUMA_POLICY[numa_policy]
    r["node_cpu_bind_policy"] = abi.NODE_BIND[node_cpu_bind_policy]
    r["numa_allocate_strategy"] = -1 if numa_allocate_strategy is None else abi.STRATEGY[numa_allocate_strategy]
    zones = numa_resources or []
    r["num_numa"] = len(zones)
    for i, z in enumerate(zones):
        r["numa_cpu"][i] = resource_value("cpu", z.get("cpu", 0))
        r["numa_mem"][i] = resource_value("memory", z.get("memory", 0))
    for name, cpus in (("reserved_cpus", reserved_cpus), ("allocated_cpus", allocated_cpus),
                       ("exclusive_pcpu_cpus", exclusive_pcpu_cpus), ("exclusive_numa_cpus", exclusive_numa_cpus)):
        w = np.zeros(abi.MAX_CPUS // 64, dtype=np.uint64)
        for c in cpus:
            w[c // 64] |= np.uint64(1) << np.uint64(c % 64)
        r[name] = w
    for i, res in (numa_allocated or {}).items():
        r["numa_alloc_cpu"][i] = resource_value("cpu", res.get("cpu", 0))
        r["numa_alloc_mem"][i] = resource_value("memory", res.get("memory", 0))
    r["cpu_amplification_ratio"] = cpu_amplification_ratio
    return n


def cpuset_of(words) -> list:
    """The cpu ids of a 256-bit mask (uint64[4])."""
    out = []
    for w, v in enumerate(np.asarray(words, dtype=np.uint64).tolist()):
        for b in range(64):
            if (v >> b) & 1:
                out.append(64 * w + b)
    return out


def make_node_device(gpus: list | None = None, has_device: bool = True, rdma: list | None = None,
                     fpga: list | None = None) -> np.ndarray:
    """DeviceShare view of one node: gpus = [{"minor": m, "healthy": True, "total": {core, memory, ratio},
    "used": {core, memory, ratio}}, ...] in koordinator.sh/gpu-* units (core / ratio percent, memory bytes).
    (ABI 17) rdma / fpga = [{"minor": m, "healthy": True, "total": percent, "used": percent}, ...]."""
    d = np.zeros(1, dtype=abi.NODE_DEVICE_DTYPE)
    r = d[0]
    r["has_device"] = int(has_device)
    for t, devs in ((abi.XTYPE_RDMA, rdma), (abi.XTYPE_FPGA, fpga)):
        for g in devs or []:
            m = int(g["minor"])
            r["x_present"][t, m] = 1
            r["x_healthy"][t, m] = int(g.get("healthy", True))
            r["x_total"][t, m] = int(g.get("total", 0))
            r["x_used"][t, m] = int(g.get("used", 0))
    for g in gpus or []:
        m = int(g["minor"])
        r["present"][m] = 1
        r["healthy"][m] = int(g.get("healthy", True))
        t, u = g.get("total", {}), g.get("used", {})
        r["total_core"][m], r["total_memory"][m], r["total_ratio"][m] = t.get("core", 0), t.get("memory", 0), t.get("ratio", 0)
        r["used_core"][m], r["used_memory"][m], r["used_ratio"][m] = u.get("core", 0), u.get("memory", 0), u.get("ratio", 0)
    return d


QUOTA_RESOURCES = ("cpu", "memory", "nvidia.com/gpu", "dcu.com/gpu", "koordinator.sh/gpu", "koordinator.sh/gpu-core",
                   "koordinator.sh/gpu-memory", "koordinator.sh/gpu-memory-ratio")


def make_quota(used_limit: dict | None = None, used: dict | None = None, min: dict | None = None,
               non_preemptible_used: dict | None = None) -> np.ndarray:
    """One ElasticQuota (kg_quota) over QUOTA_RESOURCES: {"cpu": milli, "memory": bytes, "koordinator.sh/gpu-core":
    .., ...} lists; a key absent from used_limit / min does not constrain (quotav1.LessThanOrEqual compares only the
    limit's keys)."""
    q = np.zeros(1, dtype=abi.QUOTA_DTYPE)
    r = q[0]
    for f, d, absent in (("used", used, 0), ("non_preemptible_used", non_preemptible_used, 0),
                         ("used_limit", used_limit, -1), ("min", min, -1)):
        d = d or {}
        r[f] = [int(d.get(k, absent)) for k in QUOTA_RESOURCES]
    return q


def make_pod(requests: dict | None = None, limits: dict | None = None, priority_class: str = "",
             daemonset: bool = False, nonzero: tuple | None = None, qos: str = "",
             required_cpu_bind_policy: str = "", preferred_cpu_bind_policy: str = "",
             devices: dict | None = None, quota_id: int = 0, non_preemptible: bool = False,
             preferred_cpu_exclusive_policy: str = "") -> np.ndarray:
    """One single-container pod. nonzero = schedutil.GetNonzeroRequests (100m / 200MiB defaults); qos = the
    koordinator.sh/qosClass label; *_cpu_bind_policy / preferred_cpu_exclusive_policy = the
    scheduling.koordinator.sh/resource-spec annotation."""
    p = np.zeros(1, dtype=abi.POD_DTYPE)
    r = p[0]
    req = _values(requests)
    r["requests"] = req
    r["limits"] = _values(limits)
    if nonzero is None:
        nonzero = (req[abi.RES_CPU] or 100, req[abi.RES_MEMORY] or 200 * 1024 * 1024)
    r["nonzero_requests"] = nonzero
    r["priority_class"] = abi.PRIORITY_CLASSES[priority_class]
    r["flags"] = (abi.POD_DAEMONSET if daemonset else 0) | (abi.POD_NON_PREEMPTIBLE if non_preemptible else 0)
    r["quota_id"] = quota_id  # 1 + index into the ElasticQuota table (0: the pod has no quota)
    r["qos"] = abi.QOS[qos]
    r["required_cpu_bind_policy"] = abi.BIND[required_cpu_bind_policy]
    r["preferred_cpu_bind_policy"] = abi.BIND[preferred_cpu_bind_policy]
    r["preferred_cpu_exclusive_policy"] = abi.EXCL[preferred_cpu_exclusive_policy]
    for k, v in (devices or {}).items():  # device resources: PodRequestsAndLimits of e.g. koordinator.sh/gpu-core
        r["device_requests"][abi.DEVICE_RESOURCE_SLOTS[k]] = int(v)
    return p


@dataclass
class ScheduleResult:
    suggested_host: int          # node index, -1 = FitError (unschedulable)
    score: int
    evaluated_nodes: int
    feasible_nodes: int = -1


class Scheduler:
    """SchedulePod / RunFilterPlugins / RunScorePlugins over the GPU engine."""

    def __init__(self, config: np.ndarray, capacity: int, fit: NodeResourcesFitArgs | None = None, **kw):
        """fit: the NodeResourcesFitArgs the config was built from; its RequestedToCapacityRatio shape, which kg_config
        cannot carry, is applied to the engine right after create."""
        self.config = config
        if fit is not None and fit.scoring_strategy == REQUESTED_TO_CAPACITY_RATIO:
            kw["fit_shape"] = validate_fit_shape(fit.shape if fit.shape is not None else [])
        self.engine = Engine(config, capacity, **kw)
        self._nominated = {}  # the nominator mirror: uid -> (pod record, PodPriority, node), in insertion order

    def close(self):
        self.engine.close()

    def run_filter_plugins(self, pod: np.ndarray) -> dict:
        rej, _, _ = self.engine.evaluate(pod)
        c = self.config[0]
        out = {}
        if c["fit_filter"]:
            out[NODE_RESOURCES_FIT] = np.where(rej & (abi.REJECT_FIT_PODS | abi.REJECT_FIT_CPU | abi.REJECT_FIT_MEMORY),
                                               UNSCHEDULABLE, SUCCESS)
        if c["la_filter"]:
            out[LOAD_AWARE] = np.where(rej & abi.REJECT_LOADAWARE, UNSCHEDULABLE, SUCCESS)
        return out

    def run_score_plugins(self, pod: np.ndarray) -> dict:
        _, fit, la = self.engine.evaluate(pod)
        c = self.config[0]
        out = {}
        if c["fit_score"]:
            out[NODE_RESOURCES_FIT] = fit
        if c["la_score"]:
            out[LOAD_AWARE] = la
        return out

    def debug_scores(self, topn: int, pod: np.ndarray, pod_ref: str, node_names) -> str:
        """--debug-scores N for one pod (frameworkext/debug.go:61-108): the top-N table, ranked and broken down per
        plugin on the device (kg_debug_topn), rendered with the profile's enabled Score plugins as columns."""
        rows, _ = self.engine.debug_topn(pod, topn)
        c = self.config[0]
        cols = {k: name for k, name in PLUGIN_COLUMNS.items() if c[_PLUGIN_SCORE_FIELD[k]]}
        return render_debug_table(rows, cols, pod_ref, node_names)

    def fit_error(self, pod: np.ndarray) -> FitError:
        """The FitError of a pod schedule_pod answered with -1, counted on the device (kg_pods_diagnose): call it right
        after the -1 and it is that cycle's diagnosis (an unschedulable pod leaves the state unchanged).  The reason
        strings are the engine's reason classes (REASON_STRINGS), not byte-equal to the Go messages."""
        return FitError.from_diag(self.engine.diagnose(np.asarray(pod).reshape(1))[0])

    def select_candidate(self, pod: np.ndarray, nodes, victims_per_node, priorities_per_node, starts_per_node, **kw):
        """PostFilter's DryRunPreemption + SelectCandidate for the candidate nodes the caller chose (kg_pods_preempt;
        arguments as Engine.preempt).  Returns (pick, victim pod records of the picked node in Victims.Pods order);
        pick["candidate"] = -1 and no victims when nobody can make room.  The rule is upstream's
        pickOneNodeForPreemption, ties on the lowest candidate position."""
        pick, idx, *rest = self.engine.preempt(pod, nodes, victims_per_node, priorities_per_node, starts_per_node, **kw)
        c = int(pick["candidate"])
        pods = (np.asarray(victims_per_node[c], dtype=abi.POD_DTYPE).reshape(-1)[idx] if c >= 0
                else np.zeros(0, dtype=abi.POD_DTYPE))
        return (pick, pods, *rest)

    def post_filter(self, pod: np.ndarray, priority: int, pdb_allowed=None, nodes=None, quota_rule: bool = True, **kw):
        """PostFilter over the resident bound-pod table (Engine.set_bound_pods feeds it; kg_pods_preempt_resident):
        the canPreempt selection, the MoreImportantPod order, the PDB split, the dry run and the pick on the device.
        nodes = None: every node is a candidate, as Koordinator's evaluator asks.  Returns (pick, uids of the victims on
        pick["node_idx"] in Victims.Pods order); pick["candidate"] = -1 and no uids when nobody can make room."""
        pick, uids, _idx, *rest = self.engine.preempt_resident(pod, priority, pdb_allowed, nodes, quota_rule, **kw)
        return (pick, uids, *rest)

    # -- the nominator (upstream's PodNominator): a mirror here, the table on the device -------------------------------
    def _push_nominated(self):
        ent = list(self._nominated.values())
        pods = (np.concatenate([np.asarray(p, dtype=abi.POD_DTYPE).reshape(1) for p, _, _ in ent]) if ent
                else np.zeros(0, dtype=abi.POD_DTYPE))
        self.engine.set_nominated(pods, [n for _, _, n in ent], [q for _, q, _ in ent])

    def add_nominated_pod(self, pod: np.ndarray, priority: int, node: int):
        """AddNominatedPod / UpdateNominatedPod: the pod (PostFilter's preemptor) is nominated on `node`; an entry of
        the same uid is replaced.  Every change re-sends the mirror (kg_nominated_pods_set)."""
        rec = np.array(np.asarray(pod, dtype=abi.POD_DTYPE).reshape(1)[0])
        uid = int(rec["uid"])
        old = self._nominated.pop(uid, None)
        self._nominated[uid] = (rec, int(priority), int(node))
        try:
            self._push_nominated()
        except Exception:
            del self._nominated[uid]
            if old is not None:
                self._nominated[uid] = old
            raise

    def delete_nominated_pod_if_exists(self, uid: int):
        if self._nominated.pop(int(uid), None) is not None:
            self._push_nominated()

    def nominated_pods_for_node(self, node: int):
        """NominatedPodsForNode: [(uid, PodPriority)] of the mirror's entries on `node`."""
        return [(u, q) for u, (_, q, n) in self._nominated.items() if n == int(node)]

    def _sync_nominated(self):
        """After a schedule call: the entries the device removed (their pods were placed) leave the mirror."""
        if self._nominated:
            live = set(int(u) for u in self.engine.read_nominated()[0])
            for u in [u for u in self._nominated if u not in live]:
                del self._nominated[u]

    def schedule_pods(self, pods: np.ndarray, priorities=None):
        """FIFO scheduling of `pods`; priorities (PodPriority per pod) make the call honour the nominated pods."""
        out = self.engine.schedule(pods, priorities)
        self._sync_nominated()
        return out

    def schedule_pod(self, pod: np.ndarray) -> ScheduleResult:
        node, score, _ = self.engine.schedule(np.asarray(pod).reshape(1))
        return ScheduleResult(int(node[0]), int(score[0]), self.engine.num_nodes)

    def reserve(self, pod: np.ndarray, node_idx: int):
        self.engine.add_pods(np.asarray(pod).reshape(1), [node_idx])

    def unreserve(self, pod: np.ndarray, node_idx: int):
        self.engine.remove_pods(np.asarray(pod).reshape(1), [node_idx])
