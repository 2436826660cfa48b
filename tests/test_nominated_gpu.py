"""Nominated pods on the device (kg_nominated_pods_set, kg_pods_schedule_staged_nominated, kg_pods_filter_nominated,
the resident dry run) against tests/nominated_reference.py, the plain model on the committed oracle, and against the
hand-derived known answers of tests/nominated_cases.py.  Bar: everything equal."""
from functools import lru_cache

import numpy as np
import pytest

import nominated_reference as R
import test_resident_victims as RV
from koordinator_amd import Engine, abi, framework as F, synth
from koordinator_amd.abi import KoordGPUError
from koordinator_amd.engine import Loopback
from koordinator_amd.predicates import PredicateTable
from nominated_cases import CASES, FIT, node as mk_node, pod as mk_pod
from oracle import oracle
from pick_reference import pick_candidate

GI = 1 << 30
LEVELS = np.array([0, 100, 200, 300], dtype=np.int32)
FIT_LA = F.Profile(filter=(F.NODE_RESOURCES_FIT, F.LOAD_AWARE), score={F.NODE_RESOURCES_FIT: 1, F.LOAD_AWARE: 1})
FIT_LA_NUMA = F.Profile(filter=(F.NODE_RESOURCES_FIT, F.LOAD_AWARE, F.NODE_NUMA_RESOURCE),
                        score={F.NODE_RESOURCES_FIT: 1, F.LOAD_AWARE: 1, F.NODE_NUMA_RESOURCE: 1})
BATCH_CPU = abi.RESOURCE_SLOTS["kubernetes.io/batch-cpu"]


def load(e, cluster, numa=None):
    if numa is None:
        synth.load_into(e, cluster)
    else:
        synth.load_numa_into(e, cluster, numa)


def state_equal(state, st):
    return (np.array_equal(state["requested_cpu"], st["requested"][:, abi.RES_CPU]) and
            np.array_equal(state["requested_mem"], st["requested"][:, abi.RES_MEMORY]) and
            np.array_equal(state["nonzero_cpu"], st["nonzero"][:, 0]) and
            np.array_equal(state["nonzero_mem"], st["nonzero"][:, 1]) and
            np.array_equal(state["num_pods"], st["num_pods"]) and
            np.array_equal(state["la_est_cpu"], st["la_est_all"][:, 0]) and
            np.array_equal(state["la_est_mem"], st["la_est_all"][:, 1]))


# ---- 1. the known answers, on the device ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name.replace(" ", "_"))
def test_known_answers_on_the_device(case):
    cluster = case.cluster()
    pods, prios = case.queue_arrays()
    with Engine(F.build_config(profile=case.profile), cluster.n) as e:
        load(e, cluster, np.concatenate(case.numa) if case.numa else None)
        e.set_nominated(*case.table_arrays())
        for j, i, bits, added in case.filters:
            rej, add = e.filter_nominated(pods[j:j + 1], prios[j])
            assert (int(rej[i]), int(add[i])) == (bits, added), (j, i)
        node, score, _ = e.schedule(pods, prios)
        assert list(zip(node.tolist(), score.tolist())) == case.want
        assert e.read_nominated()[0].tolist() == case.live_after


# ---- 2. device vs model on random clusters ---------------------------------------------------------------------------
@lru_cache(maxsize=None)
def world(n_nodes, numa):
    """The cluster, a 200-pod queue over 4 priority levels and 24 entries, 6 of them pods of the queue; the model's
    answer with the table and with an empty one.  Entries sit on node 0, node n - 1 and the nodes the queue uses most
    with an empty table, sized to eat most of what is free there, so that they decide placements."""
    seed = 7012 if n_nodes == 1 else 7000 + n_nodes + (50 if numa else 0)  # 7012: a node that takes 41 of the pods
    rng = np.random.default_rng(seed)
    if numa:
        cluster, nn = synth.make_numa_cluster(n_nodes, seed=seed)
        synth.amplify_numa_cluster(cluster, nn, frac=0.34, seed=seed + 1)  # ratio > 1 on a third of the nodes
        pods = synth.make_numa_pods(200, seed=seed + 2)
        cfg = F.build_config(profile=FIT_LA_NUMA)
    else:
        cluster, nn = synth.make_cluster(n_nodes, seed=seed), None
        pods = synth.make_pods(200, seed=seed + 2)
        cfg = F.build_config(profile=FIT_LA)
    # ephemeral-storage and one scalar resource, on the nodes, some bound pods and some queue pods (the engine
    # accelerates those requests in the NodeResourcesFit + LoadAware profiles only)
    aux = not numa
    if aux:
        cluster.nodes["allocatable"][:, abi.RES_EPHEMERAL] = 100 * 10**9
        cluster.nodes["allocatable"][:, BATCH_CPU] = 64000
        m = rng.random(len(cluster.existing_pods)) < 0.3
        cluster.existing_pods["requests"][m, abi.RES_EPHEMERAL] = rng.integers(1, 10, int(m.sum())) * 10**9
        for slot, frac, hi in ((abi.RES_EPHEMERAL, 0.3, 20 * 10**9), (BATCH_CPU, 0.2, 16000)):
            m = rng.random(len(pods)) < frac
            pods["requests"][m, slot] = rng.integers(1, 5, int(m.sum())) * (hi // 4)
    pods["uid"] = 1 + np.arange(len(pods))
    prios = rng.choice(LEVELS, len(pods)).astype(np.int32)
    mk = (lambda: R.make_numa(nn)) if numa else (lambda: None)
    base_node, base_score, base_st = R.schedule(cfg, cluster, pods, prios, R.Table(), mk())
    # the entries
    used, cnt = np.unique(base_node[base_node >= 0], return_counts=True)
    targets = [0, n_nodes - 1] + [int(i) for i in used[np.argsort(-cnt, kind="stable")]]
    targets = list(dict.fromkeys(targets))[:max(1, min(12, n_nodes))]
    st0 = R.initial_states(cfg, cluster)
    own = rng.choice(len(pods), 6, replace=False)
    e_pods, e_nodes, e_prios = [], [], []
    for k in range(24):
        i = targets[k % len(targets)]
        per = max(1, 24 // len(targets))
        if k < 6:  # a pod of the queue, nominated on one of the targets
            p = pods[own[k]:own[k] + 1].copy()
            q = int(prios[own[k]])
        else:
            p = np.zeros(1, dtype=abi.POD_DTYPE)
            free_c = int(cluster.nodes[i]["allocatable"][0] - st0[i]["requested"][0])
            free_m = int(cluster.nodes[i]["allocatable"][1] - st0[i]["requested"][1])
            p["requests"][0, 0] = max(0, free_c) * 9 // (10 * per)
            p["requests"][0, 1] = max(0, free_m) * 9 // (10 * per)
            p["nonzero_requests"][0] = (max(int(p["requests"][0, 0]), 100), max(int(p["requests"][0, 1]), 200 << 20))
            if aux and k % 3 == 0:
                p["requests"][0, abi.RES_EPHEMERAL] = 30 * 10**9
            if aux and k % 4 == 0:
                p["requests"][0, BATCH_CPU] = 24000
            p["uid"] = 5000 + k
            q = int(LEVELS[1 + k % 3])
        e_pods.append(p)
        e_nodes.append(i)
        e_prios.append(q)
    entries = (np.concatenate(e_pods), e_nodes, e_prios)
    table = R.Table(*entries)
    numa_state = mk()
    want_node, want_score, st = R.schedule(cfg, cluster, pods, prios, table, numa_state)
    return dict(cfg=cfg, cluster=cluster, numa=nn, pods=pods, prios=prios, entries=entries, table=table,
                want=(want_node, want_score), st=st, base=(base_node, base_score), numa_state=numa_state)


WORLDS = [(1, False), (64, False), (700, False), (64, True), (700, True)]


@pytest.mark.parametrize("n_nodes,numa", WORLDS)
def test_worlds_are_decided_by_their_entries(n_nodes, numa):
    """CPU, by the model alone: at least 10 % of the queue's placements differ from the same queue with an empty table,
    at least one entry is removed by placement and at least one survives"""
    w = world(n_nodes, numa)
    differ = int((w["want"][0] != w["base"][0]).sum())
    live = len(w["table"].stored())
    assert differ >= len(w["pods"]) // 10, differ
    assert 1 <= live < 24, live


@pytest.mark.gpu
@pytest.mark.parametrize("n_nodes,numa", WORLDS)
def test_device_matches_model(n_nodes, numa):
    """placements, totals, final node state and the table's live entries equal the model's: 1 node, 64 and 700 nodes
    (700 spans three blocks of the per-pod pass and is no multiple of its 256 threads), entries on node 0 and n - 1"""
    w = world(n_nodes, numa)
    assert {0, n_nodes - 1} <= set(w["entries"][1])
    with Engine(w["cfg"], w["cluster"].n) as e:
        load(e, w["cluster"], w["numa"])
        e.set_nominated(*w["entries"])
        node, score, _ = e.schedule(w["pods"], w["prios"])
        state, live, counters = e.read_state(), e.read_nominated(), e.nominated_counters()
        numa_dev = e.read_numa() if numa else None
    assert np.array_equal(node, w["want"][0]), np.nonzero(node != w["want"][0])[0][:5]
    assert np.array_equal(score, w["want"][1])
    assert state_equal(state, w["st"])
    assert list(zip(*(a.tolist() for a in live))) == w["table"].stored()
    if numa:  # the cpusets and per-NUMA amounts Reserve allocated: the device's NodeAllocation equals the oracle's
        for got, want in zip(numa_dev, oracle.numa_state_read(w["numa_state"]["buf"], n_nodes)):
            assert np.array_equal(got, want)
        assert (w["numa_state"]["rows"]["allocated_cpus"] != numa_dev[0]).any()  # cpusets were allocated by the queue
    assert counters["removed"] == 24 - len(w["table"].stored())
    assert counters["plain"] + counters["nominated"] == len(w["pods"])


@pytest.mark.gpu
def test_filter_nominated_matches_model():
    """reject bits and added counts on the 700-node cluster, for a pod of each priority level"""
    w = world(700, False)
    table = R.Table(*w["entries"])
    st = R.initial_states(w["cfg"], w["cluster"])
    seen = set()
    with Engine(w["cfg"], w["cluster"].n) as e:
        load(e, w["cluster"])
        e.set_nominated(*w["entries"])
        for q in LEVELS:
            j = int(np.nonzero(w["prios"] == q)[0][0])
            rej, added = e.filter_nominated(w["pods"][j:j + 1], q)
            want_rej, want_added = R.filter_nominated(w["cfg"], w["cluster"], st, w["pods"][j:j + 1], q, table)
            assert np.array_equal(added, want_added), q
            assert np.array_equal(rej, want_rej), q
            seen |= set(np.unique(want_rej[want_added > 0]).tolist())
    assert len(seen) > 1, seen  # entries that block and entries that do not


# ---- 3. renormalisation -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_taint_score_is_renormalised_over_the_narrowed_set():
    """Hand-derived.  Three 10-core nodes holding 0 / 1 / 7 cores carry 4 / 2 / 0 intolerable PreferNoSchedule taints;
    the pod asks 1 core, so NodeResourcesFit gives 90 / 80 / 20.  TaintToleration's NormalizeScore is
    100 - 100 x count / max over the FEASIBLE nodes.
      empty table:   max 4 -> 0 / 50 / 100; totals 90 / 130 / 120 -> node 1, 130.
      10-core entry on node 0 (the node holding the maximum): max 2 -> 0 / 100 over nodes 1, 2; totals 80 / 120
                     -> node 2, 120.  With the stale maximum node 1 would keep 130 and win."""
    prof = F.Profile(filter=(F.NODE_RESOURCES_FIT, F.TAINT_TOLERATION), score={F.NODE_RESOURCES_FIT: 1, F.TAINT_TOLERATION: 1})
    t = PredicateTable()
    taints = lambda k: [{"key": f"k{x}", "value": "v", "effect": "PreferNoSchedule"} for x in range(k)]  # noqa: E731
    preds = np.concatenate([t.node_row({}, taints(k)) for k in (4, 2, 0)])
    nodes = np.concatenate([mk_node(), mk_node(), mk_node()])
    metrics = np.concatenate([F.make_node_metric(present=False, node_usage=None) for _ in range(3)])
    cluster = synth.Cluster(nodes, metrics, np.concatenate([mk_pod(1, 1), mk_pod(7, 2)]), np.array([1, 2], np.int32), 10**18)
    pod = mk_pod(1, 10)
    t.fill_pod(pod, tolerations=[])
    for entries, want in ((None, (1, 130)), ((mk_pod(10, 900), [0], [100]), (2, 120))):
        with Engine(F.build_config(profile=prof), 3) as e:
            synth.load_into(e, cluster)
            e.upsert_predicates(preds)
            if entries:
                e.set_nominated(*entries)
            node, score, _ = e.schedule(pod, [50])
            assert (int(node[0]), int(score[0])) == want, entries is not None


@pytest.mark.gpu
def test_deviceshare_score_is_renormalised_over_the_narrowed_set():
    """Hand-derived.  Three 10-core nodes holding 0 / 7 / 1 cores, one GPU each with 0 / 50 / 75 % of its memory ratio
    used; the pod asks 1 core and 25 % of a GPU.  NodeResourcesFit gives 90 / 20 / 80; DeviceShare's LeastAllocated raw
    score is the free percentage after the pod, 75 / 25 / 0, normalised as 100 x raw / max over the FEASIBLE nodes.
      empty table:   max 75 -> 100 / 33 / 0; totals 190 / 53 / 80 -> node 0, 190.
      10-core entry on node 0: max 25 -> 100 / 0 over nodes 1, 2; totals 120 / 80 -> node 1, 120.  With the stale
                     maximum node 1 would get 53 and node 2 would win with 80."""
    prof = F.Profile(filter=(F.NODE_RESOURCES_FIT, F.DEVICE_SHARE), score={F.NODE_RESOURCES_FIT: 1, F.DEVICE_SHARE: 1})
    gpu = lambda used: F.make_node_device([{"minor": 0, "total": {"core": 100, "memory": 80 * GI, "ratio": 100},  # noqa: E731
                                            "used": {"core": used, "memory": used * 80 * GI // 100, "ratio": used}}])
    dev = np.concatenate([gpu(0), gpu(50), gpu(75)])
    nodes = np.concatenate([mk_node(), mk_node(), mk_node()])
    metrics = np.concatenate([F.make_node_metric(present=False, node_usage=None) for _ in range(3)])
    cluster = synth.Cluster(nodes, metrics, np.concatenate([mk_pod(7, 1), mk_pod(1, 2)]), np.array([1, 2], np.int32), 10**18)
    pod = mk_pod(1, 10, devices={"koordinator.sh/gpu-core": 25, "koordinator.sh/gpu-memory-ratio": 25})
    cfg = F.build_config(profile=prof)
    raws = [oracle.ds_score(cfg, dev[i:i + 1], pod) for i in range(3)]
    assert raws == [75, 25, 0], raws  # the raw scores the derivation above starts from
    for entries, want in ((None, (0, 190)), ((mk_pod(10, 900), [0], [100]), (1, 120))):
        with Engine(cfg, 3) as e:
            synth.load_gpu_into(e, cluster, dev)
            if entries:
                e.set_nominated(*entries)
            node, score, _ = e.schedule(pod, [50])
            assert (int(node[0]), int(score[0])) == want, entries is not None


# ---- 4. routing and the empty table -------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_routing_uses_both_paths():
    """a 210-pod queue whose first and last thirds lie above Pmax (the unchanged paths: the round engine here) and
    whose middle third lies below it (the per-pod pass with the table): results equal the model's, the counters show
    70 pods on the per-pod pass and 140 on the unchanged paths"""
    w = world(700, False)
    pods = np.concatenate([w["pods"], w["pods"][:10]]).copy()
    pods["uid"] = 1 + np.arange(len(pods))
    prios = np.full(len(pods), 1000, np.int32)
    prios[70:140] = 50
    ep, en, eq = w["entries"]
    ep = ep.copy()
    ep["uid"] = 9000 + np.arange(len(ep))  # no entry is a pod of this queue
    want_node, want_score, st = R.schedule(w["cfg"], w["cluster"], pods, prios, R.Table(ep, en, eq))
    base_node, _, _ = R.schedule(w["cfg"], w["cluster"], pods, prios, R.Table())
    assert (want_node != base_node).sum() >= 7
    with Engine(w["cfg"], w["cluster"].n) as e:
        load(e, w["cluster"])
        e.set_nominated(ep, en, eq)
        node, score, _ = e.schedule(pods, prios)
        counters, state = e.nominated_counters(), e.read_state()
    assert np.array_equal(node, want_node) and np.array_equal(score, want_score)
    assert state_equal(state, st)
    assert counters == {"plain": 140, "nominated": 70, "removed": 0}


@pytest.mark.gpu
def test_empty_table_equals_the_plain_call():
    w = world(700, False)
    cluster, pods = w["cluster"], w["pods"]
    want_node, want_score, _ = oracle.schedule_cluster(w["cfg"], cluster, pods)
    got = []
    for prios in (None, w["prios"]):
        with Engine(w["cfg"], cluster.n) as e:
            load(e, cluster)
            e.stage(pods)
            e.schedule_staged(0, len(pods), prios)
            got.append(e.fetch(0, len(pods)))
    for node, score in got:
        assert np.array_equal(node, want_node) and np.array_equal(score, want_score)


# ---- 5. the dry run -----------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def dry_run_world():
    """the 96-node shape of test_resident_victims.py without Reservation; entries on a quarter of the candidates"""
    rng = np.random.default_rng(4711)
    cluster = synth.make_cluster(96, seed=915, pods_per_node=8.0)
    cluster.nodes["allocatable"][:, abi.RES_EPHEMERAL] = 100 * 10**9
    cfg = F.build_config(profile=RV.BASE)
    table = RV.random_table(cluster, rng, 5)
    st = R.initial_states(cfg, cluster)
    e_nodes = list(range(0, 96, 4))
    e_pods = []
    for k, i in enumerate(e_nodes):
        p = np.zeros(1, dtype=abi.POD_DTYPE)
        p["requests"][0, 0] = int(cluster.nodes[i]["allocatable"][0]) * (1 + k % 4) // 8
        p["requests"][0, 1] = int(cluster.nodes[i]["allocatable"][1]) * (1 + k % 4) // 8
        p["nonzero_requests"][0] = p["requests"][0, :2]
        p["uid"] = 7000 + k
        e_pods.append(p)
    entries = (np.concatenate(e_pods), e_nodes, [int(LEVELS[1 + k % 3]) * 5 for k in range(len(e_nodes))])
    return cfg, cluster, table, st, entries


def dry_run_model(cfg, cluster, table, st, nom, pod, priority, pdb, quota_rule):
    nodes = np.arange(cluster.n, dtype=np.int32)
    refs = table.refs(nodes, pod, priority, pdb, quota_rule)
    vics, prios, starts, _, viol = table.explicit(nodes, refs)
    want = [R.select_victims(cfg, cluster, st, int(i), pod, priority, nom, vics[i], viol[i]) for i in nodes]
    off = np.zeros(cluster.n + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(v) for v in vics])
    cat = lambda per, dt: np.concatenate([np.asarray(x, dtype=dt) for x in per]) if off[-1] else np.zeros(0, dtype=dt)  # noqa: E731
    ref = pick_candidate(nodes, off, [w[0] for w in want], cat([w[1] for w in want], np.uint8), [w[2] for w in want],
                         cat(prios, np.int32), cat(starts, np.int64))
    uids = []
    if ref.candidate >= 0:
        uids = [int(vics[ref.candidate][k - int(off[ref.candidate])]["uid"]) for k in ref.victims]
    return want, refs, ref, uids


@lru_cache(maxsize=None)
def dry_run_reference():
    cfg, cluster, table, st, entries = dry_run_world()
    pdb = np.array([1, 0, 2, 1, 0], np.int32)
    runs, seen = [], {"rejected by the entry": 0, "reprieve flipped": 0}
    for cores, priority in ((48, 2000), (24, 1200), (64, 800), (16, 600)):
        pod = F.make_pod({"cpu": str(cores), "memory": f"{2 * cores}Gi"}, quota_id=0)
        pod["uid"] = 100 + cores
        for quota_rule in (True, False):
            want, refs, ref, uids = dry_run_model(cfg, cluster, table, st, R.Table(*entries), pod, priority, pdb, quota_rule)
            plain, _, _, _ = dry_run_model(cfg, cluster, table, st, R.Table(), pod, priority, pdb, quota_rule)
            for a, b in zip(want, plain):
                seen["rejected by the entry"] += a[0] != 0 and b[0] == 0
                seen["reprieve flipped"] += a[0] == 0 and b[0] == 0 and not np.array_equal(a[1], b[1])
            runs.append(dict(pod=pod, priority=priority, quota_rule=quota_rule, pdb=pdb, want=want, refs=refs,
                             record=ref.record(), uids=uids))
    return runs, seen


def test_dry_run_cases_reach_everything():
    """CPU: a candidate feasible without its entry and rejected with it, and a reprieve that flips"""
    seen = dry_run_reference()[1]
    assert all(v > 0 for v in seen.values()), seen


@pytest.mark.gpu
def test_resident_dry_run_sees_the_nominated_pods():
    cfg, cluster, table, st, entries = dry_run_world()
    runs, _ = dry_run_reference()
    nodes = np.arange(cluster.n, dtype=np.int32)
    with Engine(cfg, cluster.n) as e:
        synth.load_into(e, cluster)
        table.load(e)
        e.set_nominated(*entries)
        for r in runs:
            where = (r["priority"], r["quota_rule"])
            rej, nvio, npot, ef, er = e.select_victims_resident(r["pod"], r["priority"], r["pdb"], None, r["quota_rule"],
                                                                entries=table.entries(nodes))
            assert rej.tolist() == [int(w[0]) for w in r["want"]], where
            assert nvio.tolist() == [int(w[2]) for w in r["want"]], where
            want_f, want_r = RV.expected_entries(table, nodes, r["refs"], [w[1] for w in r["want"]])
            assert ef.tolist() == want_f.tolist() and er.tolist() == want_r.tolist(), where
            pick, uids, _, prej = e.preempt_resident(r["pod"], r["priority"], r["pdb"], None, r["quota_rule"],
                                                     want_reject=True)
            assert prej.tolist() == rej.tolist(), where
            assert tuple(int(pick[k]) for k in abi.PREEMPT_PICK_DTYPE.names) == r["record"], where
            assert uids.tolist() == r["uids"], where


@pytest.mark.gpu
def test_second_preemptor_avoids_the_first_ones_node():
    """the first preemptor is nominated on the node picked for it; a second, lower-priority preemptor of the same size
    then finds that node full and is sent elsewhere (without the entry it would be sent to the same node)"""
    cfg, cluster, table, st, _ = dry_run_world()
    pdb = np.full(5, 9, np.int32)  # budgets no victim exhausts
    first = F.make_pod({"cpu": "30", "memory": "60Gi"}, quota_id=0)
    first["uid"] = 501
    second = first.copy()
    second["uid"] = 502
    with Engine(cfg, cluster.n) as e:
        synth.load_into(e, cluster)
        table.load(e)
        p1, _, _ = e.preempt_resident(first, 2000, pdb, None, False)
        w = int(p1["node_idx"])
        assert w >= 0
        same, _, _ = e.preempt_resident(second, 1500, pdb, None, False)
        assert int(same["node_idx"]) == w  # nothing tells the second dry run about the first
        # the victims are not deleted yet: the entry fills what they would free
        e.set_nominated(first, [w], [2000])
        p2, _, _ = e.preempt_resident(second, 1500, pdb, None, False)
        want, _, ref, _ = dry_run_model(cfg, cluster, table, st, R.Table(first, [w], [2000]), second, 1500, pdb, False)
        assert int(p2["node_idx"]) == int(ref.node_idx) and int(p2["node_idx"]) != w


# ---- 6. refusals and errors ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals():
    one = (mk_pod(1, 900), [0], [100])
    nodes = np.concatenate([mk_node(), mk_node()])
    for prof, what in ((RV.RSV_FULL, "Reservation"),
                       (F.Profile(filter=(F.NODE_RESOURCES_FIT, F.POD_TOPOLOGY_SPREAD), score={F.NODE_RESOURCES_FIT: 1}),
                        "PodTopologySpread")):
        with Engine(F.build_config(profile=prof), 2) as e:
            e.upsert_nodes(nodes)
            with pytest.raises(KoordGPUError, match=what) as err:
                e.set_nominated(*one)
            assert err.value.code == abi.E_UNSUPPORTED
            e.set_nominated(np.zeros(0, dtype=abi.POD_DTYPE), [], [])  # an empty set is always fine
    with Loopback(2) as lb:
        engines = [Engine(F.build_config(profile=FIT, multi_rank="shard"), 2, rank=r, n_ranks=2, loopback=lb) for r in range(2)]
        try:
            engines[0].upsert_nodes(nodes)
            with pytest.raises(KoordGPUError, match="ranks") as err:
                engines[0].set_nominated(*one)
            assert err.value.code == abi.E_UNSUPPORTED
        finally:
            for x in engines:
                x.close()


@pytest.mark.gpu
def test_errors_and_the_old_calls():
    nodes = np.concatenate([mk_node(), mk_node()])
    metrics = np.concatenate([F.make_node_metric(present=False, node_usage=None) for _ in range(2)])
    pods = np.concatenate([mk_pod(1, 10), mk_pod(1, 11)])
    with Engine(F.build_config(profile=FIT), 4) as e:
        e.upsert_nodes(nodes)
        e.update_metrics(metrics, 10**18)
        two = np.concatenate([mk_pod(1, 900), mk_pod(1, 900)])
        for bad, match in (((two, [0, 1], [1, 1]), "nominated pod 1: uid 900 repeats entry 0"),
                           ((mk_pod(1, 0), [0], [1]), "nominated pod 0: uid 0"),
                           ((mk_pod(1, 900), [2], [1]), "nominated pod 0: node index 2"),
                           ((mk_pod(1, 900), [-1], [1]), "nominated pod 0: node index -1")):
            with pytest.raises(KoordGPUError, match=match) as err:
                e.set_nominated(*bad)
            assert err.value.code == abi.E_INVALID
        many = np.repeat(mk_pod(1, 1), abi.MAX_NOMINATED + 1)
        many["uid"] = 1 + np.arange(len(many))
        with pytest.raises(KoordGPUError, match="at most 4096") as err:
            e.set_nominated(many, np.zeros(len(many), np.int32), np.zeros(len(many), np.int32))
        assert err.value.code == abi.E_INVALID
        assert len(e.read_nominated()[0]) == 0  # a refused set leaves the table as it was
        e.set_nominated(many[:abi.MAX_NOMINATED], np.zeros(abi.MAX_NOMINATED, np.int32), np.zeros(abi.MAX_NOMINATED, np.int32))
        assert len(e.read_nominated()[0]) == abi.MAX_NOMINATED
        e.set_nominated(mk_pod(1, 900), [0], [100])
        e.stage(pods)
        for call in (lambda: e.schedule(pods), lambda: e.schedule_staged(0, 2), lambda: e.schedule(pods[:1])):
            with pytest.raises(KoordGPUError, match="kg_pods_schedule_staged_nominated") as err:
                call()
            assert err.value.code == abi.E_INVALID
        e.set_nominated(np.zeros(0, dtype=abi.POD_DTYPE), [], [])
        node, _, _ = e.schedule(pods)
        assert node.tolist() == [0, 1]


@pytest.mark.gpu
def test_scheduler_nominator_mirror():
    """Scheduler: add / delete / per-node listing, and the entries the device removed leave the mirror"""
    nodes = np.concatenate([mk_node(), mk_node()])
    metrics = np.concatenate([F.make_node_metric(present=False, node_usage=None) for _ in range(2)])
    s = F.Scheduler(F.build_config(profile=FIT), 2)
    try:
        s.engine.upsert_nodes(nodes)
        s.engine.update_metrics(metrics, 10**18)
        s.add_nominated_pod(mk_pod(8, 900), 100, 0)
        s.add_nominated_pod(mk_pod(2, 901), 100, 1)
        s.add_nominated_pod(mk_pod(3, 901), 200, 1)  # UpdateNominatedPod: replaced
        assert s.nominated_pods_for_node(1) == [(901, 200)] and s.nominated_pods_for_node(0) == [(900, 100)]
        s.delete_nominated_pod_if_exists(901)
        s.delete_nominated_pod_if_exists(12345)
        assert s.engine.read_nominated()[0].tolist() == [900]
        node, _, _ = s.schedule_pods(np.concatenate([mk_pod(4, 10), mk_pod(8, 900)]), [50, 100])
        assert node.tolist() == [1, 0]  # the low-priority pod is kept off node 0; the preemptor lands there
        assert s.nominated_pods_for_node(0) == []
    finally:
        s.close()
