"""The resolvers' dynamic LDS layouts (csrc/round_lds.h) on the device: every serial resolver against the oracle in the
shape where a mis-sized or mis-carved layout shows.

An LDS access past the allocation does not fault: reads return zero, writes are dropped.  A layout whose launch size is
too small therefore loses the tail of its last section, the modified-row bitmap, and the resolver treats a row it has
modified as unmodified.  Each case puts the decisive bit in the bitmap's last used word and fills every optional
section of the layout:

* 129 and 1,153 nodes: the highest-index node is one node into a fresh 128-node bitmap group;
* that node (`_crown`) is empty, unused and several times the size of any other, so it is the best node by a wide
  margin, and the queue starts with heavy pods (`_heavy_head`), each of which moves its integer scores;
* so the first pods of the first round — a full batch — win it one after the other, and from the second of them on
  their scores (and, once it has filled up enough, their placements) are right only if the node's bit is honoured.

Every pod's node and total score, and the final node state, are compared with the oracle's."""
import numpy as np
import pytest

import test_default_plugins as TD
import test_deviceshare_gpu as TDS
import test_numa_gpu as TN
import test_parity_gpu as TP
import test_shipped_profile as TS
from koordinator_amd import Engine, abi, framework as F, synth
from oracle import oracle

pytestmark = pytest.mark.gpu

NODES = (129, 1153)   # one node past a whole number of 128-node bitmap groups
GI = 1 << 30
HEAD = 6              # heavy pods at the head of the queue
WINS = 3              # of which at least this many must win the crowned node in the first round


def _crown(cluster, numa=None, dev=None):
    """The highest-index node, in place: four times the largest node's cpu and memory, no bound pods, no usage, no
    NUMA allocation, idle healthy GPUs."""
    last = cluster.n - 1
    alloc = cluster.nodes["allocatable"]
    alloc[last, abi.RES_CPU] = 4 * alloc[:, abi.RES_CPU].max()
    alloc[last, abi.RES_MEMORY] = 4 * alloc[:, abi.RES_MEMORY].max()
    cluster.nodes["flags"][last] = abi.NODE_VALID
    keep = cluster.existing_node != last
    cluster.existing_pods, cluster.existing_node = cluster.existing_pods[keep], cluster.existing_node[keep]
    m = cluster.metrics
    m["node_usage"][last] = 0
    for f in ("present", "has_update_time", "has_node_metric"):
        m[f][last] = 1
    m["update_time_unix_nano"][last] = synth.T0_NS
    m["node_usage_present"][last, [abi.RES_CPU, abi.RES_MEMORY]] = 1
    if numa is not None:
        for f in ("allocated_cpus", "numa_alloc_cpu", "numa_alloc_mem", "reserved_cpus"):
            numa[f][last] = 0
        numa["numa_policy"][last] = abi.NUMA_POLICY[""]
        numa["node_cpu_bind_policy"][last] = abi.NODE_BIND[""]
    if dev is not None:
        dev["has_device"][last] = 1
        dev["present"][last] = 1
        dev["healthy"][last] = 1
        dev["total_core"][last] = 100
        dev["total_ratio"][last] = 100
        dev["total_memory"][last] = synth.GPU_MEM
        for f in ("used_core", "used_ratio", "used_memory"):
            dev[f][last] = 0


def _heavy_head(pods, cpu_m=16000, mem=64 * GI):
    """The first HEAD pods of the queue, in place: plain heavy requests (a sixth of the smallest node's cpu, 3 % of
    the crowned node's), so each placement moves the winner's integer scores."""
    h = pods[:HEAD]
    h["requests"][:, abi.RES_CPU] = cpu_m
    h["requests"][:, abi.RES_MEMORY] = mem
    h["limits"][:, abi.RES_CPU] = cpu_m
    h["limits"][:, abi.RES_MEMORY] = mem
    h["nonzero_requests"][:, 0] = cpu_m
    h["nonzero_requests"][:, 1] = mem
    h["priority_class"] = abi.PRIO_PROD


def _assert_decisive(want_node, want_score, n, batch):
    """The oracle's answer has the shape the case is for: several of the first round's pods on the last node, at
    different totals."""
    first = np.flatnonzero(want_node[:batch] == n - 1)
    assert first.size >= WINS, f"only {first.size} of the first round's pods win node {n - 1}"
    assert len(set(want_score[first].tolist())) > 1, "the winner's total never moves: a stale key would go unnoticed"


# ---- resolve_round<PF, QUOTA>: Fit + LoadAware, batch_pods 64, depth 2 -------------------------------------------------
@pytest.mark.parametrize("n_quotas", [0, abi.MAX_QUOTAS], ids=["plain", "quotas"])
@pytest.mark.parametrize("n", NODES)
def test_resolve_round(n, n_quotas):
    batch = 64
    cluster = synth.make_cluster(n, seed=300 + n)
    _crown(cluster)
    pods = synth.make_pods(4 * batch, seed=301 + n)
    _heavy_head(pods)
    quotas = None
    if n_quotas:
        rng = np.random.default_rng(302 + n)
        pods["quota_id"] = rng.integers(1, n_quotas + 1, len(pods))
        pods["quota_id"][:HEAD] = n_quotas  # the heavy pods charge the table's last row
        quotas = np.zeros(n_quotas, dtype=abi.QUOTA_DTYPE)
        quotas["used_limit"] = -1
        quotas["min"] = -1
        demand = np.bincount(pods["quota_id"] - 1, weights=pods["requests"][:, abi.RES_CPU], minlength=n_quotas)
        quotas["used_limit"][:, 0] = (demand * rng.uniform(0.5, 1.5, n_quotas)).astype(np.int64)  # some run out
        quotas["used_limit"][-1, 0] = int(demand[-1])
        quotas["used_limit"][:, 1] = 1 << 50
        quotas["min"][:, :2] = quotas["used_limit"][:, :2] // 4
    cfg = F.build_config(batch_pods=batch, pods_per_wave=8, pipeline_depth=2)
    st = oracle.states(cluster.n)
    oracle.add_pods(cfg, st, cluster.existing_pods, cluster.existing_node)
    q = None if quotas is None else quotas.copy()
    want, want_score, _, _ = oracle.schedule_full(cfg, cluster.nodes, cluster.metrics, st, pods, cluster.now_ns, 8,
                                                  quotas=q)
    _assert_decisive(want, want_score, n, batch)
    with Engine(cfg, cluster.n) as e:
        synth.load_into(e, cluster)
        if quotas is not None:
            e.set_quotas(quotas)
        node, score, _ = e.schedule(pods)
        np.testing.assert_array_equal(node, want)
        np.testing.assert_array_equal(score, want_score)
        TP._assert_state_equal(e, st)
        if quotas is not None:
            assert np.array_equal(e.read_quotas(n_quotas), q)
            assert (want < 0).any()  # a quota ran out


# ---- resolve_round_numa2 (default batch, depth 2: with the prefetch section) and resolve_round_numa (depth 4) ---------
@pytest.mark.parametrize("batch,depth", [(0, 2), (15, 4)], ids=["two_wave_prefetch", "one_wave_depth4"])
@pytest.mark.parametrize("n", NODES)
def test_resolve_round_numa(n, batch, depth):
    """batch 0: kg_config's default of 32 pods, which the two-wave resolver runs with its prefetch section.  Depth 4
    needs 4 · batch < 64 slots, hence 15 pods per round; launch_resolve takes the one-wave resolver past depth 3."""
    kw = dict(batch_pods=batch, pods_per_wave=min(8, batch)) if batch else {}
    cfg = F.build_config(profile=TN.FULL_PROFILE, pipeline_depth=depth, **kw)
    cluster, numa = synth.make_numa_cluster(n, seed=310 + n)
    _crown(cluster, numa=numa)
    pods = synth.make_numa_pods(4 * (batch or 32), seed=311 + n)
    _heavy_head(pods)
    pods["qos"][:HEAD] = abi.QOS["LSR"]  # cpuset pods: 16 whole cores each
    pods["required_cpu_bind_policy"][:HEAD] = abi.BIND[""]
    pods["preferred_cpu_bind_policy"][:HEAD] = abi.BIND[""]
    st = oracle.states(cluster.n)
    oracle.add_pods(cfg, st, cluster.existing_pods, cluster.existing_node)
    node, score, _ = oracle.schedule_numa(cfg, cluster.nodes, cluster.metrics, st, oracle.numa_states(numa), pods,
                                          cluster.now_ns, n_threads=8, with_cpusets=True)
    _assert_decisive(node, score, n, batch or 32)
    TN._numa_parity(cfg, cluster, numa, pods)  # nodes, totals, cpusets, NodeAllocation, node state


# ---- resolve_round_ds: single rank, batch_pods at its bound, KG_MAX_QUOTAS quota rows --------------------------------
@pytest.mark.parametrize("n", NODES)
def test_resolve_round_ds(n):
    batch = 32  # the DeviceShare profiles' bound on batch_pods
    cluster, dev = synth.make_gpu_cluster(n, seed=320 + n)
    _crown(cluster, dev=dev)
    pods = synth.make_gpu_pods(4 * batch, seed=321 + n)
    _heavy_head(pods)
    pods["device_requests"][:HEAD] = 0
    pods["device_requests"][:HEAD, abi.DEV_GPU_CORE] = 50  # half a GPU each
    pods["device_requests"][:HEAD, abi.DEV_GPU_MEMORY_RATIO] = 50
    rng = np.random.default_rng(322 + n)
    pods["quota_id"] = rng.integers(1, abi.MAX_QUOTAS + 1, len(pods))
    quotas = np.zeros(abi.MAX_QUOTAS, dtype=abi.QUOTA_DTYPE)
    quotas["used_limit"] = -1
    quotas["min"] = -1
    demand = np.bincount(pods["quota_id"] - 1, weights=pods["requests"][:, abi.RES_CPU], minlength=abi.MAX_QUOTAS)
    quotas["used_limit"][:, 0] = np.maximum(16000 * HEAD, demand * rng.uniform(0.5, 1.5, abi.MAX_QUOTAS)).astype(np.int64)
    quotas["used_limit"][:, 2 + abi.DEV_GPU_CORE] = 400
    cfg = F.build_config(profile=TDS.PROFILE, batch_pods=batch, pods_per_wave=8)
    st = oracle.states(cluster.n)
    oracle.add_pods(cfg, st, cluster.existing_pods, cluster.existing_node)
    q, d = quotas.copy(), dev.copy()
    want, want_score, _, want_minors = oracle.schedule_full(cfg, cluster.nodes, cluster.metrics, st, pods,
                                                            cluster.now_ns, 8, devices=d, quotas=q)
    _assert_decisive(want, want_score, n, batch)
    with Engine(cfg, cluster.n) as e:
        synth.load_gpu_into(e, cluster, dev)
        e.set_quotas(quotas)
        node, score, _ = e.schedule(pods)
        np.testing.assert_array_equal(node, want)
        np.testing.assert_array_equal(score, want_score)
        np.testing.assert_array_equal(e.fetch_devices(0, len(pods)), want_minors)
        TP._assert_state_equal(e, st)
        uc, um, ur = e.read_devices()
        assert np.array_equal(uc, d["used_core"]) and np.array_equal(um, d["used_memory"])
        assert np.array_equal(ur, d["used_ratio"])
        assert np.array_equal(e.read_quotas(abi.MAX_QUOTAS), q)


# ---- xr_resolve<7>: NodeNUMAResource + DeviceShare + the upstream defaults, aux requests staged, quota rows ----------
@pytest.mark.parametrize("n", NODES)
def test_xr_resolve_every_section(n):
    batch = 32  # kXrPods: pods per exact round
    prof = F.Profile(filter=TS.PROFILE.filter + (F.TAINT_TOLERATION, F.NODE_AFFINITY),
                     score=dict(TS.PROFILE.score, **{F.TAINT_TOLERATION: 1, F.NODE_AFFINITY: 1, F.BALANCED_ALLOCATION: 1}))
    cfg = TS.config(profile=prof)
    cluster, numa, dev, rsv = synth.make_shipped_cluster(n, seed=330 + n)
    _crown(cluster, numa=numa, dev=dev)
    cluster.nodes["allocatable"][:, abi.RES_EPHEMERAL] = 400 * GI
    pods = synth.make_shipped_pods(4 * batch, seed=331 + n)
    _, preds = synth.make_predicates(cluster.n, pods, seed=332 + n)
    preds["taints_hard"][n - 1] = 0  # no taints on the crowned node
    preds["taints_soft"][n - 1] = 0
    _heavy_head(pods)
    head = pods[:HEAD]
    head["qos"] = abi.QOS["LS"]
    head["device_requests"] = 0
    for f in ("required_cpu_bind_policy", "preferred_cpu_bind_policy"):
        head[f] = abi.BIND[""]
    head["reservation_owner_mask"] = 0  # no reservation's 5000 points elsewhere
    head["reservation_flags"] = 0
    pods["requests"][1::3, abi.RES_EPHEMERAL] = 10 * GI  # ephemeral-storage requests: the aux section is staged
    quotas = synth.make_c5_quotas(pods, seed=333 + n)
    st = oracle.states(cluster.n)
    oracle.add_pods(cfg, st, cluster.existing_pods, cluster.existing_node)
    buf, r, d, q = oracle.numa_states(numa), rsv.copy(), dev.copy(), quotas.copy()
    want = oracle.schedule_resv(cfg, cluster.nodes, cluster.metrics, st, r, pods, cluster.now_ns, devices=d, quotas=q,
                                n_threads=8, with_minors=True, numa_buf=buf, with_numa=True, preds=preds)
    _assert_decisive(want[0], want[1], n, batch)
    with Engine(cfg, cluster.n) as e:
        synth.load_shipped_into(e, cluster, numa, dev, rsv, quotas)
        e.upsert_predicates(preds)
        node, score = e.schedule(pods)[:2]
        np.testing.assert_array_equal(node, want[0])
        np.testing.assert_array_equal(score, want[1])
        np.testing.assert_array_equal(e.fetch_reservations(0, len(pods)), want[2])
        np.testing.assert_array_equal(e.fetch_devices(0, len(pods)), want[3])
        np.testing.assert_array_equal(e.fetch_cpusets(0, len(pods)), want[4])
        s = e.read_state()
        np.testing.assert_array_equal(s["requested_cpu"], st["requested"][:, abi.RES_CPU])
        np.testing.assert_array_equal(s["requested_mem"], st["requested"][:, abi.RES_MEMORY])
        np.testing.assert_array_equal(s["num_pods"], st["num_pods"])
        ga, gc, gm = e.read_numa()
        wa, wc, wm = oracle.numa_state_read(buf, cluster.n)
        assert np.array_equal(ga, wa) and np.array_equal(gc, wc) and np.array_equal(gm, wm)
        got_q = e.read_quotas(len(quotas))
        assert np.array_equal(got_q["used"], q["used"])
