"""NodeResourcesBalancedAllocation on the round engine: a profile of NodeResourcesFit / LoadAware /
BalancedAllocation on one rank takes eval_round -> merge_round -> resolve_round for its batch calls, and places like
the oracle's exact pass, bit for bit.

test_round_records_on_the_routed_profile fails without the feature: the hook answers KG_E_UNSUPPORTED for a profile that
runs the exact pass."""
import numpy as np
import pytest

import balanced_cases as C
import balanced_reference as R
import nominated_reference as NR
import round_checks as RC
import round_model as M
from koordinator_amd import Engine, abi, framework, synth
from koordinator_amd.abi import KoordGPUError
from koordinator_amd.engine import Loopback
from oracle import oracle
from resolver_model import model_state

pytestmark = pytest.mark.gpu
F = framework
FIT, LA, BAL = C.FIT, C.LA, C.BAL


# ---- the wide pass and the merge (fails on an engine that keeps the profile on the exact pass) ------------------------
def test_round_records_on_the_routed_profile():
    """kg_debug_round_records on {Fit, LoadAware filter; Fit 1, LoadAware 1, Balanced 1} at 16,773 nodes: every list and
    record equals the model's keys, through the checkers of tests/round_checks.py."""
    cfg = C.parity_config("fit-la-bal-1-1-1", batch_pods=32, pods_per_wave=8)
    cl, pods = C.parity_cluster(16773), C.parity_queue(16773, 24)
    st = R.initial_states(cfg, cl)
    with Engine(cfg, cl.n) as e:
        synth.load_into(e, cl)
        e.stage(pods)
        geom, lists, recs = e.debug_round_records(0, len(pods))
    assert geom["score_bits"] == 9  # 100 * (1 + 1 + 1) = 300
    kc, moved = geom["kc"], 0
    for j in range(len(pods)):
        what = f"pod {j}"
        kv = R.keys(cfg, cl, st, pods[j:j + 1])
        RC.check_lists(lists[j], kv, geom, what)
        mlists, model = M.round_record(kv, geom)
        RC.check_record_exact(recs[j], model, kc, what, union=set(mlists.ravel().tolist()))
        RC.check_record(recs[j], kv, kc, what)
        plain = R.keys(F.build_config(profile=C.without_balanced("fit-la-bal-1-1-1")), cl, st, pods[j:j + 1])
        moved += int(kv.max(initial=0)) != 0 and R.key_node(int(kv.max())) != R.key_node(int(plain.max()))
    assert moved >= 1  # the Balanced term decides some pod's leader: the keys are not Fit + LoadAware's shifted


# ---- the rule on the device -------------------------------------------------------------------------------------------
def _oracle_scores(alloc, req, pod, resources):
    return [oracle.balanced_score(int(a[0]), int(a[1]), int(r[0]), int(r[1]), int(p[0]), int(p[1]), resources)
            for a, r, p in zip(alloc, req, pod)]


def _in_domain(alloc, req, resources):
    free = alloc - req
    ok = np.ones(len(alloc), dtype=bool)
    if resources & 1:
        ok &= (alloc[:, 0] > 0) & (alloc[:, 0] < 1 << 24) & (free[:, 0] >= -(1 << 30)) & (free[:, 0] <= alloc[:, 0])
    if resources & 2:
        ok &= (alloc[:, 1] > 0) & (alloc[:, 1] < 1 << 45) & (free[:, 1] > -(1 << 52)) & (free[:, 1] <= alloc[:, 1])
    return ok


def _boundary_triples():
    """rows around every bound of the hoisted form's domain, and pods at and past the clamps of their narrowed requests"""
    GI = C.GI
    cpu_rows = [(c, r) for c in (1, 1000, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, 0)
                for r in (0, 1, c - 1, c, c + 1, c + (1 << 30) - 1, c + (1 << 30), c + (1 << 30) + 1, -1)]
    mem_rows = [(c, r) for c in (1, 64 * GI, (1 << 45) - 1, 1 << 45, (1 << 45) + 4096, 0)
                for r in (0, 1, c - 1, c, c + 1, c + (1 << 52) - 1, c + (1 << 52), c + (1 << 52) + 1, -1)]
    pods = [(0, 0), (500, GI), (1 << 30, 1 << 52), ((1 << 30) + 1, 1 << 53), ((1 << 30) + 2, (1 << 53) + 1),
            (1 << 40, 1 << 60), (1 << 24, 1 << 45)]
    a, r, p = [], [], []
    for (cc, rc) in cpu_rows:
        for (cm, rm) in ((64 * GI, 16 * GI), (1 << 45, 5), ((1 << 45) - 1, (1 << 45) - 1)):
            for pod in pods:
                a.append((cc, cm)), r.append((rc, rm)), p.append(pod)
    for (cm, rm) in mem_rows:
        for (cc, rc) in ((8000, 2000), (1 << 24, 5), ((1 << 24) - 1, (1 << 24) - 1)):
            for pod in pods:
                a.append((cc, cm)), r.append((rc, rm)), p.append(pod)
    return np.array(a, dtype=np.int64), np.array(r, dtype=np.int64), np.array(p, dtype=np.int64)


def _random_triples(rng, n):
    """the capacities of test_fit_shape_gpu.py's boundary sweep (random below the domain's bound, small ones, whole
    GiB), one resource's sweep paired with an ordinary row of the other"""
    cpu = np.concatenate([rng.integers(1, 1 << 24, n // 2), rng.integers(1, 4096, n // 4),
                          rng.choice([1, 2, 3, 7, 100, 1000, 96000, (1 << 24) - 1, (1 << 24) - 2], n - n // 2 - n // 4)])
    mem = np.concatenate([rng.integers(1, 1 << 45, n // 2), rng.integers(1, 4096, n // 4),
                          rng.choice([g << 30 for g in (1, 3, 16, 255, 256, 1024, 4095)], n - n // 2 - n // 4)])
    rng.shuffle(mem)
    alloc = np.stack([cpu, mem], axis=1)
    req = np.stack([np.floor(cpu * rng.random(n) * 1.2).astype(np.int64), np.floor(mem * rng.random(n) * 1.2).astype(np.int64)],
                   axis=1)
    pod = np.stack([np.floor(cpu * rng.random(n) * 0.5).astype(np.int64), np.floor(mem * rng.random(n) * 0.5).astype(np.int64)],
                   axis=1)
    return alloc, req, pod


@pytest.mark.parametrize("resources", [1, 2, 3])
def test_debug_balanced(resources):
    """out_ref is oracle.balanced_score everywhere; out_hot is out_ref inside the hoisted form's domain and -1 outside
    it — on the domain's boundaries, random rows, and every triple found on the CPU whose (1 - std) * 100 lies within 2
    ulp of an integer."""
    rng = np.random.default_rng(60 + resources)
    parts = [_boundary_triples(), _random_triples(rng, 20000), C.near_integer_triples(), C.known_inputs()]
    alloc, req, pod = (np.concatenate([p[k] for p in parts]) for k in range(3))
    assert len(parts[2][0]) >= 30
    with Engine(F.build_config(), 1) as e:
        ref, hot = e.debug_balanced(alloc, req, pod, resources)
    dom = _in_domain(alloc, req, resources)
    assert dom.sum() > 0.5 * len(dom) and (~dom).sum() >= 50
    # negative Requested is not a state the engine holds; the reference-shaped routine is still checked on it
    assert ref.tolist() == _oracle_scores(alloc, req, pod, resources)
    assert np.all(hot[~dom] == -1)
    bad = np.nonzero(hot[dom] != ref[dom])[0]
    assert len(bad) == 0, (alloc[dom][bad[0]], req[dom][bad[0]], pod[dom][bad[0]], hot[dom][bad[0]], ref[dom][bad[0]])
    if resources == 3:
        assert len(set(ref.tolist())) > 40


@pytest.mark.parametrize("resources", [1, 2, 3])
@pytest.mark.parametrize("profile", ["fit-la-bal-1-1-1", "balanced-only"])
def test_eval_paths_agree(profile, resources):
    """eval_node, eval_fast and eval_hot on every (staged pod, node) of a cluster with rows outside the fast domain,
    an over-committed row and rows without cpu / memory allocatable: no mismatch"""
    cl = C.rare_cluster()
    pods = np.concatenate([C.parity_queue(129, 60), C.pod(0, 0), C.pod(200, 0), C.pod(0, 300 * C.MI)])
    cfg = C.parity_config(profile, batch_pods=32)
    cfg["balanced_resources"] = resources
    with Engine(cfg, cl.n) as e:
        synth.load_into(e, cl)
        e.stage(pods)
        assert e.debug_eval_paths() == 0
        geom, lists, recs = e.debug_round_records(0, 32)  # the wide pass on the same rows: the rare-tile path
    st = R.initial_states(cfg, cl)
    for j in range(32):
        kv = R.keys(cfg, cl, st, pods[j:j + 1])
        RC.check_lists(lists[j], kv, geom, f"pod {j}")
        RC.check_record(recs[j], kv, geom["kc"], f"pod {j}")


# ---- parity with the oracle's exact pass ------------------------------------------------------------------------------
_want = {}


def _oracle_run(key, profile, cl, pods, quotas=None, n_nodes=None):
    """oracle.schedule_resv's answer, computed once per input and shared (left unchanged); the input's claims are
    asserted on the oracle alone"""
    if key not in _want:
        cfg = C.parity_config(profile)
        node, score, st, q = R.oracle_schedule(cfg, cl, pods, quotas)
        if cl.n > 1:
            # (one node allows 110 pods and holds far fewer: "half placed" and "another node" cannot hold there)
            assert (node >= 0).sum() * 2 > len(pods), key
            plain = R.oracle_schedule(F.build_config(profile=C.without_balanced(profile)), cl, pods, quotas)[0]
            assert not np.array_equal(plain, node), key
        else:
            assert (node >= 0).any() and (node < 0).any()
        _want[key] = (node, score, st, q)
    return _want[key]


def _device_run(cfg, cl, pods, calls=None, quotas=None):
    with Engine(cfg, cl.n) as e:
        synth.load_into(e, cl)
        if quotas is not None:
            e.set_quotas(quotas)
        e.stage(pods)
        for first, count in calls or [(0, len(pods))]:
            e.schedule_staged(first, count)
        node, score = e.fetch(0, len(pods))
        return node, score, e.read_state(), (e.read_quotas(len(quotas)) if quotas is not None else None)


def _compare(got, want, what):
    node, score, state, quotas = got
    w_node, w_score, w_st, w_q = want
    bad = np.nonzero(node != w_node)[0]
    assert len(bad) == 0, f"{what}: pod {bad[0]}: node {node[bad[0]]}, the oracle's {w_node[bad[0]]} ({len(bad)} differ)"
    placed = w_node >= 0
    assert np.array_equal(score[placed], w_score[placed]), what
    ms = model_state(w_st)
    for name in ms:
        assert np.array_equal(state[name], ms[name]), f"{what}: {name}"
    if w_q is not None:
        assert np.array_equal(quotas, w_q), what


@pytest.mark.parametrize("depth", C.DEPTHS)
@pytest.mark.parametrize("profile", sorted(C.PROFILES))
@pytest.mark.parametrize("n_nodes", C.SIZES)
def test_parity_with_the_oracle(n_nodes, profile, depth):
    cl, pods = C.parity_cluster(n_nodes), C.parity_queue(n_nodes)
    want = _oracle_run((n_nodes, profile), profile, cl, pods)
    for batch in C.BATCHES:
        cfg = C.parity_config(profile, batch_pods=batch, pipeline_depth=depth)
        _compare(_device_run(cfg, cl, pods), want, f"{n_nodes} nodes, {profile}, depth {depth}, batch {batch}")


def test_score_bits_of_the_large_weight():
    """LoadAware 1 + Balanced 1000: totals up to 100,100 need 17 bits, and the rounds run at that width"""
    cfg = C.parity_config("la-bal-1000", batch_pods=16)
    cl = C.parity_cluster(129)
    with Engine(cfg, cl.n) as e:
        synth.load_into(e, cl)
        e.stage(C.parity_queue(129, 4))
        assert e.debug_round_records(0, 4)[0]["score_bits"] == 17


@pytest.mark.parametrize("profile", sorted(C.PROFILES))
def test_parity_two_pod_calls(profile):
    """calls of 2 pods keep the per-pod exact pass; the rest of the queue takes the round engine on the state they left"""
    cl, pods = C.parity_cluster(1100), C.parity_queue(1100)
    want = _oracle_run((1100, profile), profile, cl, pods)
    calls = [(f, 2) for f in range(0, 60, 2)] + [(60, 100), (160, 2), (162, 1), (163, len(pods) - 163)]
    _compare(_device_run(C.parity_config(profile, batch_pods=38, pipeline_depth=2), cl, pods, calls), want,
             f"{profile}, 2-pod calls")


@pytest.mark.parametrize("batch,depth", [(16, 3), (38, 2), (64, 1)])
def test_parity_aux_requests(batch, depth):
    cl, pods = C.aux_inputs()
    assert (pods["requests"][:, abi.RES_EPHEMERAL] > 0).sum() > 100
    want = _oracle_run(("aux",), "fit-la-bal-1-1-1", cl, pods)
    plain = _oracle_run((1100, "fit-la-bal-1-1-1"), "fit-la-bal-1-1-1", C.parity_cluster(1100), C.parity_queue(1100))
    assert not np.array_equal(want[0], plain[0])  # the ephemeral-storage requests decide some placements
    _compare(_device_run(C.parity_config("fit-la-bal-1-1-1", batch_pods=batch, pipeline_depth=depth), cl, pods), want,
             f"aux requests, batch {batch}, depth {depth}")


@pytest.mark.parametrize("batch,depth", [(16, 3), (38, 2), (64, 1)])
def test_parity_with_quotas(batch, depth):
    cl, pods, quotas = C.quota_inputs()
    want = _oracle_run(("quota",), "fit-la-bal-1-1-1", cl, pods, quotas)
    rejected = sum(1 for j in range(len(pods)) if want[0][j] < 0 and pods["quota_id"][j] > 0)
    assert rejected >= 10 and (want[3]["used"] > 0).any()
    _compare(_device_run(C.parity_config("fit-la-bal-1-1-1", batch_pods=batch, pipeline_depth=depth), cl, pods,
                         quotas=quotas), want, f"quotas, batch {batch}, depth {depth}")


def test_nominated_pods(monkeypatch):
    """schedule_staged(..., priorities) against nominated_reference composed with this profile's keys: 64 nodes, 8
    entries, two of them preemptors that come through the queue"""
    cl = synth.make_cluster(64, seed=51)
    rng = np.random.default_rng(52)
    entries = C.parity_queue(129, 8)
    entries["uid"] = 900 + np.arange(8)
    e_nodes, e_prio = rng.choice(64, 8, replace=False).astype(np.int32), np.full(8, 100, np.int32)
    queue = C.parity_queue(129, 60)
    queue["uid"] = 10 + np.arange(60)
    queue[7], queue[30] = entries[2], entries[5]
    prio = rng.choice(np.array([50, 100, 150], np.int32), 60)
    cfg = C.parity_config("fit-bal", batch_pods=16)
    monkeypatch.setattr(NR, "plain_keys", lambda cfg, cluster, st, pod, numa=None: R.keys(cfg, cluster, st, pod))
    table = NR.Table(entries, e_nodes, e_prio)
    want_node, want_score, want_st = NR.schedule(cfg, cl, queue, prio, table)
    monkeypatch.undo()
    plain_node, _, _ = NR.schedule(F.build_config(profile=C.without_balanced("fit-bal")), cl, queue, prio,
                                   NR.Table(entries, e_nodes, e_prio))
    assert not np.array_equal(want_node, plain_node) and (want_node >= 0).sum() >= 30
    with Engine(cfg, cl.n) as e:
        synth.load_into(e, cl)
        e.set_nominated(entries, e_nodes, e_prio)
        e.stage(queue)
        e.schedule_staged(0, len(queue), prio)
        node, score = e.fetch(0, len(queue))
        state = e.read_state()
        live = e.read_nominated()[0].tolist()
    assert np.array_equal(node, want_node)
    assert np.array_equal(score[want_node >= 0], want_score[want_node >= 0])
    assert live == [u for u, _, _ in table.stored()]
    ms = model_state(want_st)
    for col in ms:
        assert np.array_equal(state[col], ms[col]), col


# ---- the resolver alone -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.SCENARIOS))
def test_resolver_scenarios(name):
    """resolve_round through kg_debug_resolve on the two scenarios a monotone resolver answers wrongly: out_keys and the
    published list are the sequential answer's"""
    s = C.SCENARIOS[name]()
    cfg = C.scenario_config(s, depth=2)
    snap = R.initial_states(cfg, s.cl)
    prev = [[(s.queue[pi:pi + 1], nd) for pi, nd in lst] for lst in s.prev]
    want, published, st = R.sequential_answer(cfg, s.cl, snap, s.queue[:s.nb], prev)
    assert R.skip_rule_answer(cfg, s.cl, snap, s.queue[:s.nb], prev) != want
    with Engine(cfg, s.cl.n) as e:
        synth.load_into(e, s.cl)
        e.stage(s.queue)
        dev = e.debug_resolve(0, s.nb, s.prev)
        state = e.read_state()
    assert dev["error"] == 0 and dev["consumed"] == s.nb and dev["poison"] == 0
    assert [int(k) for k in dev["out_keys"]] == want, [R.key_node(int(k)) for k in dev["out_keys"]]
    assert dev["list"].tolist() == published
    assert dev["slow"] == (s.nb if s.prev else s.nb - 1)  # every pod re-scores the modified rows once there are any
    ms = model_state(st)
    for col in ms:
        assert np.array_equal(state[col], ms[col]), col


# ---- routing stays put where it must ----------------------------------------------------------------------------------
def test_prod_usage_variant_keeps_the_exact_pass():
    cl, pods = C.parity_cluster(1100), C.parity_queue(1100)
    kw = dict(profile=C.PROFILES["fit-la-bal-1-1-1"], la=F.LoadAwareSchedulingArgs(score_according_prod_usage=True))
    node, score, st, _ = R.oracle_schedule(F.build_config(**kw), cl, pods)
    cfg = F.build_config(batch_pods=38, **kw)
    _compare(_device_run(cfg, cl, pods), (node, score, st, None), "ScoreAccordingProdUsage")
    with Engine(cfg, cl.n) as e:
        synth.load_into(e, cl)
        e.stage(pods[:4])
        with pytest.raises(KoordGPUError) as err:
            e.debug_round_records(0, 4)  # not routed: the hook still refuses the profile
        assert err.value.code == abi.E_UNSUPPORTED


def test_two_ranks_keep_the_exact_pass():
    """an engine created with n_ranks = 2 (loopback) is not routed, and places like the oracle on every rank"""
    import threading
    cl, pods = C.parity_cluster(129), C.parity_queue(129, 120)
    want = R.oracle_schedule(C.parity_config("fit-la-bal-1-1-1"), cl, pods)
    cfg = C.parity_config("fit-la-bal-1-1-1", batch_pods=16)
    out, errs = [None, None], []
    with Loopback(2) as g:
        engines = [Engine(cfg, cl.n, rank=r, n_ranks=2, loopback=g) for r in range(2)]
        try:
            for e in engines:
                synth.load_into(e, cl)
                e.stage(pods)

            def work(r):
                try:
                    engines[r].schedule_staged(0, len(pods))
                    node, score = engines[r].fetch(0, len(pods))
                    out[r] = (node, score, engines[r].read_state(), None)
                except Exception as ex:  # surfaced below
                    errs.append(ex)

            ts = [threading.Thread(target=work, args=(r,)) for r in range(2)]
            for t in ts:
                t.start()
            for t in ts:
                t.join()
            assert not errs, errs
            with pytest.raises(KoordGPUError) as err:
                engines[0].debug_round_records(0, 4)
            assert err.value.code == abi.E_UNSUPPORTED
        finally:
            for e in engines:
                e.close()
    for rank in range(2):
        _compare(out[rank], want, f"rank {rank} of 2")


def test_other_strategies_still_refuse_balanced():
    prof = C.PROFILES["fit-la-bal-1-1-1"]
    with pytest.raises(KoordGPUError) as err:
        Engine(F.build_config(profile=prof, fit=F.NodeResourcesFitArgs(scoring_strategy="MostAllocated")), 64)
    assert err.value.code == abi.E_UNSUPPORTED
    with Engine(F.build_config(profile=prof), 64) as e:
        with pytest.raises(KoordGPUError) as err:
            e.set_fit_shape([(0, 0), (100, 10)])
        assert err.value.code == abi.E_UNSUPPORTED


def test_per_pod_entry_points_answer_as_the_exact_pass():
    """kg_pods_evaluate_reservation, kg_pods_diagnose and kg_debug_topn on a routed profile, after a batch the round
    engine placed: each against the model's keys on the oracle's state"""
    profile = "fit-la-bal-1-1-1"
    cl, pods = C.parity_cluster(1100), C.parity_queue(1100)
    cfg = C.parity_config(profile, batch_pods=38)
    _, _, st, _ = _oracle_run((1100, profile), profile, cl, pods)
    probes = np.concatenate([C.parity_queue(129, 6), C.pod(10_000_000, 0)])
    with Engine(cfg, cl.n) as e:
        synth.load_into(e, cl)
        e.upsert_predicates(np.zeros(cl.n, dtype=abi.NODE_PRED_DTYPE))  # legal: the predicate table exists
        e.schedule(pods)
        for j in range(len(probes)):
            kv = R.keys(cfg, cl, st, probes[j:j + 1])
            feas = kv != 0
            ev = e.evaluate_reservation(probes[j])
            assert np.array_equal(ev["pass"] != 0, feas), j
            # `base` is the Fit + LoadAware part: this entry point has never added the default plugins' terms
            kp = oracle.node_keys(cfg, cl.nodes, cl.metrics, st, probes[j:j + 1], cl.now_ns, 0, cl.n)
            assert np.array_equal(ev["base"][feas], (kp[feas] >> np.uint64(32)).astype(np.int64)), j
            rows, n_feas = e.debug_topn(probes[j], 5)
            top = np.sort(kv[feas])[::-1][:5]
            assert n_feas == int(feas.sum())
            assert rows["node_idx"].tolist() == [R.key_node(int(k)) for k in top]
            assert rows["total"].tolist() == [int(k) >> 32 for k in top]
            cols = [abi.RES_CPU, abi.RES_MEMORY]
            for row in rows:
                i = int(row["node_idx"])
                bs = R.balanced_scores(cl.nodes["allocatable"][i:i + 1][:, cols], st["requested"][i:i + 1][:, cols],
                                       R.pod_request(probes[j:j + 1]))
                assert int(row["plugin"][abi.PL_BALANCED]) == int(bs[0])
        diag = e.diagnose(probes)
        for j in range(len(probes)):
            assert int(diag[j]["feasible"]) == int((R.keys(cfg, cl, st, probes[j:j + 1]) != 0).sum())
        assert int(diag[-1]["feasible"]) == 0
