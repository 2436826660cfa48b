"""Inputs for the NodeNUMAResource tests across CPU topologies: a topology table, a cluster that mixes
its rows, a queue of wide cpuset requests and a census of what an oracle run exercised.  No GPU here: the census reads
the inputs and the oracle's answer only, so its counts say what the device tests are run on, not what the device did.

The table (sockets, NUMA nodes per socket, cores per NUMA node, cpus per core; cpu = buildCPUTopology numbering):
every entry has <= 256 cpus, <= 8 topology NUMA nodes and cpus_per_core <= 2 (what the engine's ingest accepts)."""
import numpy as np

from koordinator_amd import abi, framework as F, synth
from oracle import oracle

GI, MI = synth.GI, synth.MI

TOPOLOGIES = [
    (2, 1, 26, 2),   # 104 cpus: the reference's own (resource_manager_test.go:541); NUMA node 1 = 52-103 straddles 64
    (2, 1, 24, 2),   # 96: NUMA node 1 = 48-95 straddles 64
    (2, 1, 33, 2),   # 132: NUMA node 1 = 66-131 crosses 64 and 128
    (1, 1, 100, 2),  # 200: one NUMA node over four words, not a multiple of 64
    (1, 3, 20, 2),   # 120: three NUMA nodes, the middle one (40-79) straddles
    (2, 2, 12, 1),   # 48: SMT off, inside one word
    (2, 2, 20, 1),   # 80: SMT off, NUMA node 3 = 60-79 straddles
    (4, 1, 16, 2),   # 128: four sockets, 32 cpus per NUMA node
    (1, 1, 32, 2),   # 64: the word branch of make_view at one word per node
    (2, 1, 32, 2),   # 128: the same, two nodes
    (2, 1, 64, 2),   # 256: synth.make_numa_cluster's, as a control
    (2, 2, 32, 2),   # 256: synth.make_numa_cluster's, as a control
    (4, 2, 8, 2),    # 128: 8 topology NUMA nodes (no zones reported: num_numa 0, NUMA policy none)
    (8, 1, 16, 2),   # 256: 8 sockets (the same)
    (1, 1, 3, 2),    # 6: tiny
    (1, 1, 1, 1),    # 1: tiny
]
SIZES = (1, 2, 3, 4, 5, 7, 8, 16, 24, 26, 33, 48, 52, 64, 100)  # cpus a cpuset pod asks for
BIND_KINDS = ("none", "required FullPCPUs", "required SpreadByPCPUs", "preferred SpreadByPCPUs", "preferred FullPCPUs")
_INV = {name: {v: k for k, v in d.items() if k not in ("None", "Default")}
        for name, d in (("bind", abi.BIND), ("excl", abi.EXCL), ("policy", abi.NUMA_POLICY), ("node_bind", abi.NODE_BIND))}

FULL_PROFILE = F.Profile(filter=(F.NODE_RESOURCES_FIT, F.LOAD_AWARE, F.NODE_NUMA_RESOURCE),
                         score={F.NODE_RESOURCES_FIT: 1, F.LOAD_AWARE: 1, F.NODE_NUMA_RESOURCE: 1})


def n_cpus(topo):
    s, n, k, t = topo
    return s * n * k * t


def zones_of(topo):
    """NUMA zones the node reports: its topology NUMA nodes, or none when there are more than the engine holds."""
    z = topo[0] * topo[1]
    return z if z <= abi.MAX_NUMA else 0


def words(cpus):
    w = np.zeros(abi.MAX_CPUS // 64, dtype=np.uint64)
    for c in cpus:
        w[c // 64] |= np.uint64(1) << np.uint64(c % 64)
    return w


def topo_of(row):
    return tuple(int(row[k]) for k in ("sockets", "nodes_per_socket", "cores_per_node", "cpus_per_core"))


def make_mixed_cluster(n_nodes, seed, fill=0.7, topologies=TOPOLOGIES):
    """(Cluster, kg_node_numa[n]): node i has topology i mod len(topologies), so neighbouring rows (one wide-pass tile,
    one resolver launch) differ in size and in the make_view branch they take.  Allocatable cpu = cpus x 1000, memory
    4 GiB per cpu (at least 64 GiB); zones split both evenly.  allocated_cpus is drawn per cpu (not per core) at a
    per-node density in [0, fill], so partially free cores exist; 30 % of nodes reserve 1-3 free cpus anywhere; on
    40 % of nodes 30 % / 20 % of the allocated cpus are held under PCPULevel / NUMANodeLevel.  numa_alloc_cpu = the
    allocated cpus of each zone x 1000, numa_alloc_mem 0-40 % of the zone.  Policies as synth.make_numa_cluster (an
    8-node topology has no zones and so no NUMA policy).  One bound pod per node carries the cpusets' cpu (+ 0-10 %
    shared cpu) and the zones' memory in NodeInfo; NodeMetric usage is 0-60 % cpu / 0-90 % memory of the node's own
    size."""
    rng = np.random.default_rng(seed)
    n = n_nodes
    nodes = np.zeros(n, dtype=abi.NODE_DTYPE)
    nodes["allowed_pods"] = 250
    nodes["flags"] = abi.NODE_VALID
    nodes["custom_usage_thresholds"] = -1
    nodes["custom_prod_usage_thresholds"] = -1
    numa = np.zeros(n, dtype=abi.NODE_NUMA_DTYPE)
    numa["has_topology"] = 1
    u = rng.random(n)
    policy = np.select([u < 0.5, u < 0.7, u < 0.85], [abi.NUMA_POLICY[""], abi.NUMA_POLICY["BestEffort"],
                       abi.NUMA_POLICY["Restricted"]], abi.NUMA_POLICY["SingleNUMANode"])
    u = rng.random(n)
    numa["node_cpu_bind_policy"] = np.select([u < 0.10, u < 0.15], [abi.NODE_BIND["FullPCPUsOnly"],
                                             abi.NODE_BIND["SpreadByPCPUs"]], abi.NODE_BIND[""])
    u = rng.random(n)
    numa["numa_allocate_strategy"] = np.select([u < 0.1, u < 0.2], [abi.STRATEGY["LeastAllocated"],
                                               abi.STRATEGY["MostAllocated"]], -1)
    req_cpu = np.zeros(n, dtype=np.int64)
    req_mem = np.zeros(n, dtype=np.int64)
    for i in range(n):
        topo = topologies[i % len(topologies)]
        total, z = n_cpus(topo), zones_of(topo)
        mem = max(64, 4 * total) * GI
        nodes["allocatable"][i, abi.RES_CPU] = total * 1000
        nodes["allocatable"][i, abi.RES_MEMORY] = mem
        r = numa[i]
        r["sockets"], r["nodes_per_socket"], r["cores_per_node"], r["cpus_per_core"] = topo
        r["num_numa"] = z
        r["numa_policy"] = policy[i] if z else abi.NUMA_POLICY[""]
        held = np.flatnonzero(rng.random(total) < (1 - rng.random() ** 2) * fill)
        r["allocated_cpus"] = words(held)
        free = np.setdiff1d(np.arange(total), held)
        if rng.random() < 0.3 and len(free):
            r["reserved_cpus"] = words(rng.choice(free, min(len(free), int(rng.integers(1, 4))), replace=False))
        if rng.random() < 0.4:
            pick = rng.random(len(held))
            r["exclusive_pcpu_cpus"] = words(held[pick < 0.3])
            r["exclusive_numa_cpus"] = words(held[(pick >= 0.3) & (pick < 0.5)])
        zm = np.zeros(0, dtype=np.int64)
        if z:
            r["numa_cpu"][:z] = total * 1000 // z
            r["numa_mem"][:z] = mem // z
            r["numa_alloc_cpu"][:z] = np.bincount(held // (total // z), minlength=z)[:z] * 1000
            zm = np.floor(rng.random(z) * 0.4 * (mem // z) / MI).astype(np.int64) * MI
            r["numa_alloc_mem"][:z] = zm
        shared = int(rng.random() * 0.1 * total * 1000)
        # (a one-cpu node has no shared pool beside its one cpuset cpu: with any shared request a free one could
        # never pass Fit for a 1-cpu cpuset pod)
        req_cpu[i] = len(held) * 1000 + (shared if total > 1 else 0)
        req_mem[i] = int(zm.sum()) if z else int(rng.random() * 0.4 * mem / MI) * MI
    ex = np.zeros(n, dtype=abi.POD_DTYPE)
    ex["requests"][:, abi.RES_CPU] = req_cpu
    ex["requests"][:, abi.RES_MEMORY] = req_mem
    ex["limits"] = ex["requests"]
    ex["nonzero_requests"][:, 0] = np.maximum(req_cpu, 100)
    ex["nonzero_requests"][:, 1] = np.maximum(req_mem, 200 * MI)
    ex["priority_class"] = abi.PRIO_PROD
    keep = (req_cpu > 0) | (req_mem > 0)
    cpu, mem = nodes["allocatable"][:, abi.RES_CPU], nodes["allocatable"][:, abi.RES_MEMORY]
    metrics = np.zeros(n, dtype=abi.METRIC_DTYPE)
    has = rng.random(n) < 0.95
    metrics["present"] = has
    metrics["has_update_time"] = has
    metrics["has_node_metric"] = has
    metrics["update_time_unix_nano"] = np.where(has, synth.T0_NS, 0)
    metrics["node_usage"][:, abi.RES_CPU] = np.where(has, np.floor(rng.random(n) * 0.6 * cpu), 0).astype(np.int64)
    metrics["node_usage"][:, abi.RES_MEMORY] = np.where(has, np.floor(rng.random(n) * 0.9 * mem / MI), 0).astype(np.int64) * MI
    metrics["node_usage_present"][:, abi.RES_CPU] = has
    metrics["node_usage_present"][:, abi.RES_MEMORY] = has
    cluster = synth.Cluster(nodes, metrics, ex[keep], np.flatnonzero(keep).astype(np.int32), synth.T0_NS + 10 * 10**9)
    return cluster, numa


def amplify_mixed(cluster, numa, seed):
    """cpu amplification ratio 1.5 / 2.0 on a third of the nodes, in place, as synth.amplify_numa_cluster leaves them:
    node allocatable cpu and every zone's cpu amplified (ceil of whole cpus), the bound pods' allocations unchanged."""
    rng = np.random.default_rng(seed)
    on = rng.random(cluster.n) < 1 / 3
    ratio = np.where(on, rng.choice(np.array([1.5, 2.0]), cluster.n), 0.0)
    amp = lambda v, r: np.where(r > 1, np.ceil(v.astype(np.float64) * r), v).astype(np.int64)
    cluster.nodes["allocatable"][:, abi.RES_CPU] = amp(cluster.nodes["allocatable"][:, abi.RES_CPU] // 1000, ratio) * 1000
    numa["numa_cpu"] = amp(numa["numa_cpu"] // 1000, ratio[:, None]) * 1000
    numa["cpu_amplification_ratio"] = ratio
    return ratio


def make_wide_pods(n_pods, seed):
    """synth.make_numa_pods' mix (60 % LSR + 10 % LSE koord-prod cpuset pods, 25 % LS, 4 % BE koord-batch, 1 % zero
    requests) with cpuset requests from SIZES — below, between and above the per-node and per-socket sizes of
    TOPOLOGIES, odd ones included —, the five BIND_KINDS equally likely and preferred exclusive policy none 50 % /
    PCPULevel 30 % / NUMANodeLevel 20 %; memory 256Mi-8Gi, and none for a third of the pods: with a memory request
    the merged hint is never wider than memory's preferred single NUMA node (policy.go:127-185), so only a cpu-only
    pod can get an affinity of several NUMA nodes stored."""
    rng = np.random.default_rng(seed)
    p = np.zeros(n_pods, dtype=abi.POD_DTYPE)
    u = rng.random(n_pods)
    cpuset = u < 0.7
    cpu = np.where(cpuset, rng.choice(np.array(SIZES, dtype=np.int64), n_pods) * 1000,
                   rng.choice(np.array([250, 500, 1500, 2000, 4000], dtype=np.int64), n_pods))
    mem = rng.choice(np.array([0, 0, 256, 1024, 4096, 8192], dtype=np.int64), n_pods) * MI
    zero = u >= 0.99
    cpu[zero] = 0
    mem[zero] = 0
    p["requests"][:, abi.RES_CPU] = cpu
    p["requests"][:, abi.RES_MEMORY] = mem
    p["limits"] = p["requests"]
    p["nonzero_requests"][:, 0] = np.where(cpu > 0, cpu, 100)
    p["nonzero_requests"][:, 1] = np.where(mem > 0, mem, 200 * MI)
    p["priority_class"] = np.where((u >= 0.95) & (u < 0.99), abi.PRIO_BATCH, abi.PRIO_PROD)
    p["qos"] = np.select([u < 0.6, u < 0.7, u < 0.95], [abi.QOS["LSR"], abi.QOS["LSE"], abi.QOS["LS"]], abi.QOS["BE"])
    b = rng.integers(0, len(BIND_KINDS), n_pods)
    p["required_cpu_bind_policy"] = np.where(cpuset, np.select([b == 1, b == 2], [abi.BIND["FullPCPUs"],
                                             abi.BIND["SpreadByPCPUs"]], abi.BIND[""]), abi.BIND[""])
    p["preferred_cpu_bind_policy"] = np.where(cpuset, np.select([b == 3, b == 4], [abi.BIND["SpreadByPCPUs"],
                                              abi.BIND["FullPCPUs"]], abi.BIND[""]), abi.BIND[""])
    e = rng.random(n_pods)
    p["preferred_cpu_exclusive_policy"] = np.where(cpuset, np.select([e < 0.5, e < 0.8], [abi.EXCL[""],
                                                   abi.EXCL["PCPULevel"]], abi.EXCL["NUMANodeLevel"]), abi.EXCL[""])
    return p


def is_cpuset_pod(pods):
    return ((pods["qos"] == abi.QOS["LSR"]) | (pods["qos"] == abi.QOS["LSE"])) & (pods["priority_class"] == abi.PRIO_PROD) \
        & (pods["requests"][:, abi.RES_CPU] > 0)


def bind_kind(pod):
    rq, pf = int(pod["required_cpu_bind_policy"]), int(pod["preferred_cpu_bind_policy"])
    if rq:
        return "required " + _INV["bind"][rq]
    return "preferred " + _INV["bind"][pf] if pf else "none"


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's run and the census
# ---------------------------------------------------------------------------------------------------------------------
def initial_state(cfg, cluster):
    st = oracle.states(cluster.n)
    oracle.add_pods(cfg, st, cluster.existing_pods, cluster.existing_node)
    return st


def oracle_run(cfg, cluster, numa, pods, n_threads=8):
    """The whole queue in one call: dict(node, score, cpus, nalloc, st, buf)."""
    st = initial_state(cfg, cluster)
    buf = oracle.numa_states(numa)
    node, score, cpus, _, nalloc = oracle.schedule_full(cfg, cluster.nodes, cluster.metrics, st, pods, cluster.now_ns,
                                                        n_threads, numa_buf=buf, with_numa_alloc=True)
    return dict(node=node, score=score, cpus=cpus, nalloc=nalloc, st=st, buf=buf)


def oracle_steps(cfg, cluster, numa, pods):
    """The queue one pod per call, keeping what each placement saw: dict(node, score, cpus, nalloc, st, buf) as
    oracle_run plus `before` — per placed pod the chosen node's kg_node_numa row and NodeInfo (requested cpu, memory)
    just before its Reserve —, `affinity`, the mask Filter stored for that node (-1: nil), and `single_numa_rejects`:
    per cpuset pod, at its turn, the SingleNUMANode nodes whose Filter rejects it while the same node under BestEffort
    admits it."""
    st = initial_state(cfg, cluster)
    buf = oracle.numa_states(numa)
    rows = numa.copy()
    n = len(pods)
    out = dict(node=np.full(n, -1, np.int32), score=np.zeros(n, np.int64),
               cpus=np.zeros((n, abi.MAX_CPUS // 64), np.uint64), nalloc=None, before=[None] * n,
               affinity=np.full(n, -2, np.int64), st=st, buf=buf)
    recs = []
    alloc = cluster.nodes["allocatable"]
    single = np.flatnonzero(numa["numa_policy"] == abi.NUMA_POLICY["SingleNUMANode"])
    out["single_numa_rejects"] = np.zeros(n, np.int32)
    cs = is_cpuset_pod(pods)

    def evaluate(row, k, j):
        return oracle.numa_eval(cfg, row, pods[k:k + 1], (int(st["requested"][j, abi.RES_CPU]),
                                int(st["requested"][j, abi.RES_MEMORY])),
                                (int(alloc[j, abi.RES_CPU]), int(alloc[j, abi.RES_MEMORY])))

    for k in range(n):
        if cs[k]:  # SingleNUMANode nodes that reject the pod where the same node under BestEffort admits it
            for j in single:
                if not evaluate(rows[j:j + 1], k, j)[0]:
                    loose = rows[j:j + 1].copy()
                    loose["numa_policy"] = abi.NUMA_POLICY["BestEffort"]
                    out["single_numa_rejects"][k] += evaluate(loose, k, j)[0]
        prev = st["requested"].copy()
        node, score, cpus, _, nalloc = oracle.schedule_full(cfg, cluster.nodes, cluster.metrics, st, pods[k:k + 1],
                                                            cluster.now_ns, 4, numa_buf=buf, with_numa_alloc=True)
        out["node"][k], out["score"][k], out["cpus"][k] = node[0], score[0], cpus[0]
        recs.append(nalloc[0].copy())
        j = int(node[0])
        if j < 0:
            continue
        req = (int(prev[j, abi.RES_CPU]), int(prev[j, abi.RES_MEMORY]))
        out["before"][k] = (rows[j:j + 1].copy(), req)
        ok, _, mask = oracle.numa_eval(cfg, rows[j:j + 1], pods[k:k + 1], req,
                                       (int(alloc[j, abi.RES_CPU]), int(alloc[j, abi.RES_MEMORY])))
        assert ok, f"pod {k}: the oracle placed it on node {j}, whose Filter rejects it"
        out["affinity"][k] = mask
        rows[j] = oracle.numa_state_export(buf, j, rows[j])[0]
    out["nalloc"] = np.array(recs)
    return out


def effective_bind(cfg, row, pod):
    """(policy takeCPUs runs with, required?) for a cpuset pod on a node (plugin.go:556-576 after PreFilter :220-270)."""
    default = int(cfg[0]["numa_default_cpu_bind_policy"])
    rq, pf = int(pod["required_cpu_bind_policy"]), int(pod["preferred_cpu_bind_policy"])
    bind = pf if pf not in (abi.BIND[""], abi.BIND["Default"]) else default
    if rq == abi.BIND["Default"]:
        rq = default
    if rq:
        bind = rq
    nb = int(row["node_cpu_bind_policy"])
    if nb == abi.NODE_BIND["SpreadByPCPUs"]:
        bind = abi.BIND["SpreadByPCPUs"]
    elif nb == abi.NODE_BIND["FullPCPUsOnly"]:
        bind = abi.BIND["FullPCPUs"]
    return bind, bool(rq)


def _cores(cpus, cpc):
    by = {}
    for c in cpus:
        by.setdefault(c // cpc, []).append(c)
    return by


def shortcut_holds(cfg, row, pod, rec):
    """The single-NUMA shortcut of the device's take_cpus, restated over cpu lists: every takeCPUs call of this
    Reserve (one per NUMA node of the allocation record `rec`, or one over all available cpus) asks FullPCPUs (or the
    node has one cpu per core) without an exclusive policy, for no more than a NUMA node holds, from cpus that all lie
    in one NUMA node and whose whole free cores cover the request."""
    topo = topo_of(row)
    cpc, per_node = topo[3], topo[2] * topo[3]
    bind, required = effective_bind(cfg, row, pod)
    if not (bind == abi.BIND["FullPCPUs"] or cpc == 1) or int(pod["preferred_cpu_exclusive_policy"]) != 0:
        return False
    busy = set(F.cpuset_of(row["allocated_cpus"])) | set(F.cpuset_of(row["reserved_cpus"]))
    avail = [c for c in range(n_cpus(topo)) if c not in busy]
    if required:
        by = _cores(avail, cpc)
        if bind == abi.BIND["FullPCPUs"]:
            avail = [c for c in avail if len(by[c // cpc]) == cpc]
        elif bind == abi.BIND["SpreadByPCPUs"]:
            avail = [c for c in avail if c == by[c // cpc][0]]
    need = int(pod["requests"][abi.RES_CPU]) // 1000
    calls = []
    if int(rec[0]):
        for i in range(abi.MAX_NUMA):
            if (int(rec[0]) >> i) & 1:
                part = [c for c in avail if c // per_node == i]
                calls.append((part, min(len(part), int(rec[1 + i]) // 1000)))
    else:
        calls.append((avail, need))
    for part, k in calls:
        if k < 1:
            continue
        by = _cores(part, cpc)
        whole = sum(len(v) for v in by.values() if len(v) == cpc)
        if k > per_node or len({c // per_node for c in part}) != 1 or whole < k:
            return False
    return True


def census(cfg, cluster, numa, pods, res):
    """Counts of what the run `res` (oracle_steps) exercised, per cpuset pod: dict class name -> count, plus
    "topology (s, n, k, t)" -> cpuset placements on that topology."""
    from collections import Counter
    c = Counter()
    cs = is_cpuset_pod(pods)
    for k in np.flatnonzero(cs):
        pod = pods[k]
        need = int(pod["requests"][abi.RES_CPU]) // 1000
        c["bind " + bind_kind(pod)] += 1
        c["excl " + (_INV["excl"][int(pod["preferred_cpu_exclusive_policy"])] or "none")] += 1
        if res["single_numa_rejects"][k]:
            c["rejected by a node under SingleNUMANode only"] += 1
        if res["node"][k] < 0:
            c["unschedulable"] += 1
            continue
        c["placed"] += 1
        row, _ = res["before"][k]
        row = row[0]
        topo = topo_of(row)
        s, n, kk, cpc = topo
        per_node, per_socket = kk * cpc, n * kk * cpc
        c[f"topology {topo}"] += 1
        c[f"cpc {cpc}"] += 1
        busy = set(F.cpuset_of(row["allocated_cpus"])) | set(F.cpuset_of(row["reserved_cpus"]))
        free = [x for x in range(n_cpus(topo)) if x not in busy]
        node_free = max(np.bincount([x // per_node for x in free], minlength=1))
        socket_free = max(np.bincount([x // per_socket for x in free], minlength=1))
        c["request " + ("<= a NUMA node's free cpus" if need <= node_free else
                        "<= a socket's free cpus" if need <= socket_free else "<= the node's free cpus")] += 1
        c["request " + ("<= per-node size" if need <= per_node else
                        "<= per-socket size" if need <= per_socket else "> per-socket size")] += 1
        got = F.cpuset_of(res["cpus"][k])
        c["cpuset in " + ("several mask words" if len({x // 64 for x in got}) > 1 else "one mask word")] += 1
        c["cpuset on " + ("several NUMA nodes" if len({x // per_node for x in got}) > 1 else "one NUMA node")] += 1
        c["cpuset on " + ("several sockets" if len({x // per_socket for x in got}) > 1 else "one socket")] += 1
        partial = cpc == 2 and any(len(v) == 1 for v in _cores(free, cpc).values())
        c["node " + ("with" if partial else "without") + " partially free cores"] += 1
        c["single-NUMA shortcut " + ("holds" if shortcut_holds(cfg, row, pod, res["nalloc"][k]) else "does not hold")] += 1
        pol = _INV["policy"][int(row["numa_policy"])] or "none"
        aff = int(res["affinity"][k])
        c[f"policy {pol}"] += 1
        c[f"policy {pol} affinity " + ("nil" if aff < 0 else f"of {bin(aff).count('1')} NUMA nodes")] += 1
        if len(got) > need:
            c["cpuset larger than the request"] += 1
    return c


# ---------------------------------------------------------------------------------------------------------------------
# the failure message of the device tests
# ---------------------------------------------------------------------------------------------------------------------
def describe(pods, k, numa, answers):
    """Pod k's request and policies, and per answer (name, node, cpuset words) the node's topology and policies."""
    pod = pods[k]
    out = [f"pod {k}: cpu {int(pod['requests'][abi.RES_CPU])}m memory {int(pod['requests'][abi.RES_MEMORY]) >> 20}Mi "
           f"qos {int(pod['qos'])} bind {bind_kind(pod)} "
           f"exclusive {_INV['excl'][int(pod['preferred_cpu_exclusive_policy'])] or 'none'}"]
    for name, node, cpus in answers:
        node = int(node)
        line = f"  {name}: node {node}"
        if node >= 0:
            r = numa[node]
            line += (f" topology {topo_of(r)} NUMA policy {_INV['policy'][int(r['numa_policy'])] or 'none'} node bind "
                     f"{_INV['node_bind'][int(r['node_cpu_bind_policy'])] or 'none'} strategy "
                     f"{int(r['numa_allocate_strategy'])} ratio {float(r['cpu_amplification_ratio'])} cpus "
                     f"{F.cpuset_of(cpus)}")
        out.append(line)
    return "\n".join(out)


def first_difference(pods, numa, want_node, want_cpus, got_node, got_cpus, want_score=None, got_score=None):
    """None, or the message for the first pod whose placement, total or cpuset differs."""
    bad = (np.asarray(got_node) != np.asarray(want_node)) | (np.asarray(got_cpus) != np.asarray(want_cpus)).any(axis=1)
    if want_score is not None:
        bad |= np.asarray(got_score) != np.asarray(want_score)
    bad = np.flatnonzero(bad)
    if bad.size == 0:
        return None
    k = int(bad[0])
    msg = describe(pods, k, numa, [("oracle", want_node[k], want_cpus[k]), ("device", got_node[k], got_cpus[k])])
    if want_score is not None:
        msg += f"\n  totals: oracle {int(want_score[k])} device {int(got_score[k])}"
    return f"{bad.size} pods differ, the first:\n{msg}"
