"""NodeNUMAResource on the device across CPU topologies: the HIP engine, through the C ABI, against the
oracle restatement (oracle/numa.c) on clusters that mix the topologies of tests/numa_topology_cases.py — NUMA nodes and
sockets that straddle a 64-cpu mask word, SMT off, three and eight NUMA nodes, eight sockets, partially free cores,
requests wider than a NUMA node or a socket.  tests/test_numa_topology_cases.py asserts, on the oracle alone, what
these inputs exercise.

Bar: bit-exact, as tests/test_numa_gpu.py — Filter verdicts, scores and stored affinities of every (pod, node) pair;
placements, totals and cpusets of every pod; the final NodeAllocation and NodeInfo / LoadAware node state.  A mismatch
names the first differing pod's request and policies, the node's topology and policies and both answers.

One engine is alive at a time and no round pipeline is deeper than 3."""
import numpy as np
import pytest

import numa_topology_cases as C
import test_golden_numa as TG
import test_numa_topology_cases as TC
import test_parity_gpu as TP
from koordinator_amd import Engine, abi, framework as F, synth
from oracle import oracle

pytestmark = pytest.mark.gpu

N_NODES, N_PODS = TC.N_NODES, TC.N_PODS


def _workload(kind):
    """A fresh (cluster, numa, pods) of the loose / tight cluster, the one the census describes."""
    w = TC.LOOSE if kind == "loose" else TC.TIGHT
    cluster, numa = C.make_mixed_cluster(N_NODES, w["seed"], w["fill"])
    return cluster, numa, C.make_wide_pods(N_PODS, w["seed"] + 1000)


def _engine(cfg, cluster, numa):
    e = Engine(cfg, cluster.n)
    synth.load_numa_into(e, cluster, numa)
    return e


def _assert_numa_state(e, numa, buf):
    ga, gc, gm = e.read_numa()
    wa, wc, wm = oracle.numa_state_read(buf, len(numa))
    bad = np.flatnonzero((ga != wa).any(axis=1) | (gc != wc).any(axis=1) | (gm != wm).any(axis=1))
    if bad.size:
        i = int(bad[0])
        raise AssertionError(
            f"{bad.size} nodes differ in NodeAllocation, the first: node {i} topology {C.topo_of(numa[i])}\n"
            f"  oracle cpus {F.cpuset_of(wa[i])} cpu {wc[i].tolist()} memory {wm[i].tolist()}\n"
            f"  device cpus {F.cpuset_of(ga[i])} cpu {gc[i].tolist()} memory {gm[i].tolist()}")


def _assert_answers(e, pods, numa, w, first=0, count=None):
    count = len(pods) - first if count is None else count
    node, score = e.fetch(first, count)
    cpus = e.fetch_cpusets(first, count)
    s = slice(first, first + count)
    msg = C.first_difference(pods[s], numa, w["node"][s], w["cpus"][s], node, cpus, w["score"][s], score)
    assert msg is None, msg


def _parity(cfg, cluster, numa, pods, run=None):
    """_numa_parity's bar (tests/test_numa_gpu.py): placements, totals, cpusets, read_numa state, node state."""
    w = C.oracle_run(cfg, cluster, numa, pods)
    with _engine(cfg, cluster, numa) as e:
        e.stage(pods)
        if run is None:
            e.schedule_staged(0, len(pods))
        else:
            run(e)
        _assert_answers(e, pods, numa, w)
        _assert_numa_state(e, numa, w["buf"])
        TP._assert_state_equal(e, w["st"])
    return w


# ---------------------------------------------------------------------------------------------------------------------
# Filter, Score and the stored affinity of every (pod, node) pair
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["loose", "tight"])
def test_evaluate_numa_all_pairs(kind):
    cfg = F.build_config(profile=C.FULL_PROFILE)
    cluster, numa, pods = _workload(kind)
    cs = np.flatnonzero(C.is_cpuset_pod(pods))
    pick = np.concatenate([cs[:20], np.flatnonzero(~C.is_cpuset_pod(pods))[:4]])  # 24 pods, 20 of them cpuset pods
    st = C.initial_state(cfg, cluster)
    alloc = cluster.nodes["allocatable"]
    with _engine(cfg, cluster, numa) as e:
        got = [e.evaluate_numa(pods[k:k + 1]) for k in pick]
    for k, (ok, sc, af) in zip(pick, got):
        for i in range(cluster.n):
            want = oracle.numa_eval(cfg, numa[i:i + 1], pods[k:k + 1],
                                    (st["requested"][i, abi.RES_CPU], st["requested"][i, abi.RES_MEMORY]),
                                    (alloc[i, abi.RES_CPU], alloc[i, abi.RES_MEMORY]))
            have = (bool(ok[i]), int(sc[i]), int(af[i]))
            assert have == want, (f"(passes, score, affinity) device {have} oracle {want}\n"
                                  + C.describe(pods, int(k), numa, [("node", i, numa[i]["allocated_cpus"])]))


# ---------------------------------------------------------------------------------------------------------------------
# scheduling parity
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch,depth", [(16, 2), (16, 3), (1, 0)])
@pytest.mark.parametrize("kind", ["loose", "tight"])
def test_schedule_parity(kind, batch, depth):
    """batch 16 depth 2 is the two-wave resolver, depth 3 the three-deep pipeline, batch 1 the serial resolver."""
    cfg = F.build_config(profile=C.FULL_PROFILE, batch_pods=batch, pods_per_wave=min(8, batch), pipeline_depth=depth)
    cluster, numa, pods = _workload(kind)
    w = _parity(cfg, cluster, numa, pods)
    assert (w["cpus"] != 0).any(axis=1).sum() > 300


def test_single_pod_calls():
    cfg = F.build_config(profile=C.FULL_PROFILE)
    cluster, numa, pods = _workload("loose")
    pods = pods[:60]

    def run(e):
        for i in range(len(pods)):
            e.schedule_staged(i, 1)

    _parity(cfg, cluster, numa, pods, run)


@pytest.mark.parametrize("variant", ["score_only", "most_allocated", "numa_only_spread_default"])
def test_profile_variants(variant):
    """tests/test_numa_gpu.py::test_c4_profile_variants' profiles on the loose cluster.

    `score_only` has no NodeNUMAResource Filter, so nothing rejects an odd request under a required FullPCPUs policy:
    on a node of three or more sockets takeCPUs can give such a pod one cpu more, all whole cores, and Score and
    Reserve succeed (pod 22: 33 cpus asked, 34 held on node 189, an (8, 1, 16, 2) node)."""
    if variant == "score_only":
        prof = F.Profile(filter=(F.NODE_RESOURCES_FIT,), score={F.NODE_RESOURCES_FIT: 1, F.NODE_NUMA_RESOURCE: 2})
        cfg = F.build_config(profile=prof)
    elif variant == "most_allocated":
        numa_args = F.NodeNUMAResourceArgs(scoring_strategy="MostAllocated", numa_scoring_strategy="MostAllocated")
        cfg = F.build_config(profile=C.FULL_PROFILE, numa=numa_args)
    else:
        numa_args = F.NodeNUMAResourceArgs(default_cpu_bind_policy="SpreadByPCPUs")
        cfg = F.build_config(profile=TG.NUMA_PROFILE, numa=numa_args)
    cluster, numa, pods = _workload("loose")
    _parity(cfg, cluster, numa, pods)


def test_amplified():
    """cpu amplification ratio 1.5 / 2.0 on a third of the loose cluster's nodes."""
    cfg = F.build_config(profile=C.FULL_PROFILE, batch_pods=16, pods_per_wave=8)
    cluster, numa, pods = _workload("loose")
    ratio = C.amplify_mixed(cluster, numa, seed=TC.LOOSE["seed"] + 2000)
    assert 40 < (ratio > 1).sum() < 100
    w = _parity(cfg, cluster, numa, pods)
    on = ratio[np.maximum(w["node"], 0)] > 1
    assert ((w["cpus"] != 0).any(axis=1) & (w["node"] >= 0) & on).sum() > 50  # cpusets on amplified nodes


def test_unreserve_round_trip():
    """300 pods, Unreserve of a random half of the placed ones (numa_release on cpusets over several mask words), 300
    more: the same sequence on the oracle."""
    cfg = F.build_config(profile=C.FULL_PROFILE, batch_pods=16, pods_per_wave=8)
    cluster, numa, pods = _workload("loose")
    a = 300
    st, buf = C.initial_state(cfg, cluster), oracle.numa_states(numa)
    n1, s1, c1, _, r1 = oracle.schedule_full(cfg, cluster.nodes, cluster.metrics, st, pods[:a], cluster.now_ns, 8,
                                             numa_buf=buf, with_numa_alloc=True)
    m = (n1 >= 0) & (np.random.default_rng(5).random(a) < 0.5)
    wide = [j for j in np.flatnonzero(m) if len({c // 64 for c in F.cpuset_of(c1[j])}) > 1]
    assert len(wide) > 20  # released cpusets that span mask words
    for j in np.flatnonzero(m):
        oracle.unreserve(cfg, st, pods[j], n1[j], numa_buf=buf, cpus=c1[j], numa_alloc=r1[j])
    n2, s2, c2, _ = oracle.schedule_full(cfg, cluster.nodes, cluster.metrics, st, pods[a:], cluster.now_ns, 8,
                                         numa_buf=buf)
    with _engine(cfg, cluster, numa) as e:
        e.stage(pods)
        e.schedule_staged(0, a)
        _assert_answers(e, pods, numa, dict(node=n1, score=s1, cpus=c1), 0, a)
        e.unreserve(0, a, m)
        e.schedule_staged(a, len(pods) - a)
        w = dict(node=np.concatenate([n1, n2]), score=np.concatenate([s1, s2]), cpus=np.concatenate([c1, c2]))
        _assert_answers(e, pods, numa, w, a, len(pods) - a)
        _assert_numa_state(e, numa, buf)
        TP._assert_state_equal(e, st)


RSV_PROFILE = F.Profile(filter=C.FULL_PROFILE.filter + (F.RESERVATION,),
                        score={**C.FULL_PROFILE.score, F.RESERVATION: 5000})


def test_exact_pass_with_reservations():
    """The mixed NUMA rows under a profile that also holds Reservation: the per-pod exact pass and its Reserve
    (xr_reserve).  No reservation holds a cpuset."""
    cfg = F.build_config(profile=RSV_PROFILE)
    cluster, numa, pods = _workload("loose")
    cluster, rsv = synth.make_rsv_cluster(cluster.n, seed=TC.LOOSE["seed"] + 3000, cluster=cluster)
    pods = synth.make_rsv_pods(300, seed=TC.LOOSE["seed"] + 3001, base=pods[:300].copy())
    assert not rsv["cpus"].any()
    st, buf, r = C.initial_state(cfg, cluster), oracle.numa_states(numa), rsv.copy()
    node, score, slot, cpus, _ = oracle.schedule_resv(cfg, cluster.nodes, cluster.metrics, st, r, pods, cluster.now_ns,
                                                      n_threads=8, numa_buf=buf, with_numa=True)
    assert (slot >= 0).sum() > 5 and (cpus != 0).any(axis=1).sum() > 100
    with Engine(cfg, cluster.n) as e:
        synth.load_numa_into(e, cluster, numa)
        e.upsert_reservations(rsv)
        e.stage(pods)
        e.schedule_staged(0, len(pods))
        _assert_answers(e, pods, numa, dict(node=node, score=score, cpus=cpus))
        np.testing.assert_array_equal(e.fetch_reservations(0, len(pods)), slot)
        _assert_numa_state(e, numa, buf)
        TP._assert_state_equal(e, st)


# ---------------------------------------------------------------------------------------------------------------------
# the reference's Allocate rows and the pinned extra-cpu case, through Reserve on one node
# ---------------------------------------------------------------------------------------------------------------------
def _one_node(cfg, node, nn):
    e = Engine(cfg, 1)
    e.upsert_nodes(node)
    e.upsert_numa(nn)
    return e


@pytest.mark.parametrize("c", TC.ALLOC["cases"], ids=TC._alloc_id)
def test_allocate_row_device(c):
    cfg, node, nn, pod, hint = TC.allocate_case(c)
    with _one_node(cfg, node, nn) as e:
        ok, _, mask = e.evaluate_numa(pod)
        assert ok[0] and int(mask[0]) == hint, c["source_line"]  # Filter stores the row's hint
        e.stage(pod)
        e.schedule_staged(0, 1)
        placed, _ = e.fetch(0, 1)
        assert placed[0] == 0 and F.cpuset_of(e.fetch_cpusets(0, 1)[0]) == c["want"], c["source_line"]
        _, cpu, _ = e.read_numa()
    assert (cpu[0] - nn["numa_alloc_cpu"][0]).tolist() == TC.want_numa_cpu(c), c["source_line"]


def test_one_cpu_more_than_asked_device():
    cfg, nn, pod, want = TC.extra_cpu_case()
    with _one_node(cfg, F.make_node({"cpu": "32", "memory": str(1 << 40)}), nn) as e:
        e.stage(pod)
        e.schedule_staged(0, 1)
        assert e.fetch(0, 1)[0][0] == 0 and F.cpuset_of(e.fetch_cpusets(0, 1)[0]) == want


@pytest.mark.parametrize("held_more,placed", [([], True), ([10, 11, 12, 13, 14, 15], False)])
def test_odd_required_full_pcpus_without_filter(held_more, placed):
    """The extra-cpu case under a required FullPCPUs policy in a profile without the plugin's Filter: 11 cpus asked,
    the 12 whole-core cpus held and a positive Score — and, with socket 1 held as well (one socket left to pass over),
    a Score of 0 and a Reserve that fails.  Against the oracle."""
    c = TC.EXTRA_CPU_CASE
    prof = F.Profile(filter=(F.NODE_RESOURCES_FIT,), score={F.NODE_RESOURCES_FIT: 1, F.NODE_NUMA_RESOURCE: 2})
    cfg = F.build_config(profile=prof)
    nn = F.make_node_numa(*c["topo"], allocated_cpus=sorted(c["alloc"] + held_more))
    node = F.make_node({"cpu": "32", "memory": str(1 << 40)})
    pod = F.make_pod({"cpu": str(c["need"])}, priority_class="koord-prod", qos="LSR", required_cpu_bind_policy="FullPCPUs")
    st, buf = oracle.states(1), oracle.numa_states(nn)
    wn, ws, wc, _ = oracle.schedule_full(cfg, node, F.make_node_metric(present=False), st, pod, 0, 1, numa_buf=buf)
    assert (wn[0] == 0) == placed and F.cpuset_of(wc[0]) == (c["want"] if placed else [])
    with _one_node(cfg, node, nn) as e:
        _, sc, _ = e.evaluate_numa(pod)
        want_sc = oracle.numa_eval(cfg, nn, pod, (0, 0), (32000, 1 << 40))[1]
        assert int(sc[0]) == want_sc and (want_sc > 0) == placed
        e.stage(pod)
        e.schedule_staged(0, 1)
        gn, gs = e.fetch(0, 1)
        assert (int(gn[0]), int(gs[0]), F.cpuset_of(e.fetch_cpusets(0, 1)[0])) == (int(wn[0]), int(ws[0]), F.cpuset_of(wc[0]))
        _assert_numa_state(e, nn, buf)


@pytest.mark.parametrize("topo", [(8, 1, 16, 2), (4, 2, 8, 2)], ids=["8x1x16x2", "4x2x8x2"])
def test_odd_requests_on_random_whole_core_states(topo):
    """The kernel's odd_full_take against the oracle: 48 nodes of one topology whose free cpus are whole cores at random
    (per-node density at random, so from no socket to every socket holds the request), a profile without the plugin's
    Filter, and odd requests under a required FullPCPUs policy; Score of every (pod, node) pair."""
    prof = F.Profile(filter=(F.NODE_RESOURCES_FIT,), score={F.NODE_RESOURCES_FIT: 1, F.NODE_NUMA_RESOURCE: 2})
    cfg = F.build_config(profile=prof)
    rng = np.random.default_rng(21)
    n, total = 48, C.n_cpus(topo)
    numa = np.concatenate([F.make_node_numa(*topo, allocated_cpus=[c for core in np.flatnonzero(
        rng.random(total // 2) < rng.random()) for c in (2 * core, 2 * core + 1)]) for _ in range(n)])
    nodes = np.concatenate([F.make_node({"cpu": str(total), "memory": str(1 << 40)})] * n)
    needs = (3, 5, 7, 17, 33, 35, 49, 65)
    pods = [F.make_pod({"cpu": str(k)}, priority_class="koord-prod", qos="LSR", required_cpu_bind_policy="FullPCPUs")
            for k in needs]
    want = np.array([[oracle.numa_eval(cfg, numa[i:i + 1], pod, (0, 0), (total * 1000, 1 << 40))[1] for i in range(n)]
                     for pod in pods])
    assert 20 <= (want > 0).sum() <= want.size - 100  # takes that end on whole cores, and more that do not
    with Engine(cfg, n) as e:
        e.upsert_nodes(nodes)
        e.upsert_numa(numa)
        got = np.array([e.evaluate_numa(pod)[1] for pod in pods])
    bad = np.argwhere(got != want)
    assert bad.size == 0, (f"{len(bad)} (pod, node) pairs differ, the first: {needs[bad[0][0]]} cpus on node {bad[0][1]}, "
                           f"free cpus {sorted(set(range(total)) - set(F.cpuset_of(numa[bad[0][1]]['allocated_cpus'])))}: "
                           f"device Score {got[tuple(bad[0])]} oracle {want[tuple(bad[0])]}")


# ---------------------------------------------------------------------------------------------------------------------
# one node per topology, pod by pod
# ---------------------------------------------------------------------------------------------------------------------
def _hand_node(idx, topo):
    """One node of `topo` with a hand-set state: every cpu whose id is a multiple of 5, or 3 more than a multiple of 14,
    is held by bound pods — about a quarter of the cpus, which leaves single-free cores all along the id range (on both
    sides of cpu 64 where the topology reaches it: cores 4|5, 11|10, 14|15 ... 59|58, 61|60, 64|65, 71|70) — and the
    highest free cpu is reserved.  The two tiny topologies keep cpus to give: (1,1,3,2) holds cpu 3 alone and reserves
    cpu 5, the one-cpu node holds and reserves nothing.  Zones (where the topology has at most four NUMA nodes) under BestEffort for every other
    topology, no NUMA policy for the rest."""
    total, z = C.n_cpus(topo), C.zones_of(topo)
    held = [c for c in range(total) if c % 5 == 0 or c % 14 == 3] if total >= 16 else [3][:total // 6]
    free = [c for c in range(total) if c not in held]
    per = total // z if z else total
    zones = [{"cpu": f"{per * 1000}m", "memory": str(64 << 30)}] * z
    allocated = {i: {"cpu": f"{1000 * sum(1 for c in held if c // per == i)}m"} for i in range(z)}
    return F.make_node_numa(*topo, numa_policy="BestEffort" if z and idx % 2 else "", numa_resources=zones,
                            allocated_cpus=held, reserved_cpus=free[-1:] if len(free) > 1 else [],
                            numa_allocated=allocated, exclusive_pcpu_cpus=held[::3], exclusive_numa_cpus=held[1::7])


def _hand_pods(topo):
    """Eight cpu-only LSR pods: small and odd requests under every bind kind and exclusive policy, and one request a
    cpu wider than a NUMA node (a quarter of it where the topology has a single NUMA node)."""
    per_node = topo[2] * topo[3]
    wide = per_node + 1 if topo[0] * topo[1] > 1 else max(1, per_node // 4)
    spec = [(3, "", "SpreadByPCPUs", ""), (4, "FullPCPUs", "", ""), (5, "", "", "PCPULevel"),
            (2, "SpreadByPCPUs", "", "NUMANodeLevel"), (wide, "", "FullPCPUs", ""), (7, "", "FullPCPUs", ""),
            (6, "", "SpreadByPCPUs", ""), (1, "", "", "")]
    return np.concatenate([F.make_pod({"cpu": str(n)}, priority_class="koord-prod", qos="LSR",
                                      required_cpu_bind_policy=rq, preferred_cpu_bind_policy=pf,
                                      preferred_cpu_exclusive_policy=ex) for n, rq, pf, ex in spec])


# which of the eight steps place on each hand node (the oracle's answer, fixed here so that a hand state which places
# nothing on a topology cannot pass unnoticed)
HAND_PLACED = {
    (2, 1, 26, 2): "11111101", (2, 1, 24, 2): "11111010", (2, 1, 33, 2): "11111111", (1, 1, 100, 2): "11111111",
    (1, 3, 20, 2): "11111111", (2, 2, 12, 1): "11110011", (2, 2, 20, 1): "11111111", (4, 1, 16, 2): "11111111",
    (1, 1, 32, 2): "11111111", (2, 1, 32, 2): "11111111", (2, 1, 64, 2): "11111111", (2, 2, 32, 2): "11111111",
    (4, 2, 8, 2): "11111111", (8, 1, 16, 2): "11111111",
    (1, 1, 3, 2): "10001000",  # cpus {0, 2, 4}, then {1}
    (1, 1, 1, 1): "00001000",  # the 1-cpu request takes cpu 0: the one Reserve any test runs on the one-cpu topology
}


@pytest.mark.parametrize("idx", range(len(C.TOPOLOGIES)), ids=["x".join(map(str, t)) for t in C.TOPOLOGIES])
def test_one_node_pod_by_pod(idx):
    topo = C.TOPOLOGIES[idx]
    cfg = F.build_config(profile=TG.NUMA_PROFILE)
    nn, pods = _hand_node(idx, topo), _hand_pods(topo)
    node = F.make_node({"cpu": str(C.n_cpus(topo)), "memory": str(1 << 40)})
    metric = F.make_node_metric(present=False)
    st, buf = oracle.states(1), oracle.numa_states(nn)
    want = [oracle.schedule_full(cfg, node, metric, st, pods[k:k + 1], 0, 1, numa_buf=buf) for k in range(len(pods))]
    assert [int(w[0][0]) == 0 for w in want] == [ch == "1" for ch in HAND_PLACED[topo]], topo  # Reserve runs on every row
    assert all(w[2][0].any() for w in want if int(w[0][0]) == 0)
    with _one_node(cfg, node, nn) as e:
        e.stage(pods)
        for k, (wn, ws, wc, _) in enumerate(want):
            e.schedule_staged(k, 1)
            gn, gs = e.fetch(k, 1)
            gc = e.fetch_cpusets(k, 1)
            assert (int(gn[0]), int(gs[0]), F.cpuset_of(gc[0])) == (int(wn[0]), int(ws[0]), F.cpuset_of(wc[0])), (
                f"topology {topo} step {k}: device (node, total, cpus) first, oracle second\n"
                + C.describe(pods, k, nn, [("oracle", wn[0], wc[0]), ("device", gn[0], gc[0])]))
        _assert_numa_state(e, nn, buf)


# ---------------------------------------------------------------------------------------------------------------------
# shapes the engine does not hold are refused at upsert
# ---------------------------------------------------------------------------------------------------------------------
def test_topologies_beyond_the_engine_are_refused():
    cfg = F.build_config(profile=TG.NUMA_PROFILE)
    zones8 = F.make_node_numa(4, 2, 8, 2)
    zones8["num_numa"] = 8                      # more zones than the device's per-NUMA arrays hold
    # fewer zones than an 8-node topology has NUMA nodes, under a NUMA policy: the view would count the first four only
    zones2 = F.make_node_numa(4, 2, 8, 2, numa_policy="BestEffort", numa_resources=[{"cpu": "64", "memory": "64Gi"}] * 2)
    zones4 = F.make_node_numa(8, 1, 16, 2, numa_policy="SingleNUMANode", numa_resources=[{"cpu": "64", "memory": "64Gi"}] * 4)
    with Engine(cfg, 1) as e:
        e.upsert_nodes(F.make_node({"cpu": "256", "memory": str(1 << 40)}))
        for nn in (zones8, zones2, zones4, F.make_node_numa(2, 1, 65, 2), F.make_node_numa(16, 1, 8, 2), F.make_node_numa(2, 8, 8, 2),
                   F.make_node_numa(2, 1, 8, 4)):
            with pytest.raises(abi.KoordGPUError) as err:
                e.upsert_numa(nn)
            assert err.value.code == abi.E_UNSUPPORTED, C.topo_of(nn[0])
        e.upsert_numa(F.make_node_numa(8, 1, 16, 2))  # the largest shape it does hold
