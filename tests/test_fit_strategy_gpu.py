"""NodeResourcesFit ScoringStrategy MostAllocated on the device: the division-free quotients, the two
evaluation paths, the rule's known answers, bit-exact parity of the round engine with the plain model of
tests/fit_strategy_reference.py (placements, totals, node state, quotas), the resolver alone on the three scenarios a
monotone resolver gets wrong, nominated pods, and the refusals.

Every test that sets the strategy fails on an engine that ignores the config word: it would place by LeastAllocated."""
import numpy as np
import pytest

import fit_strategy_cases as C
import fit_strategy_reference as R
import nominated_reference as NR
from koordinator_amd import Engine, abi, framework, synth
from koordinator_amd.abi import KoordGPUError
from resolver_model import model_state

pytestmark = pytest.mark.gpu
F = framework
MOST_ARGS = F.NodeResourcesFitArgs(scoring_strategy="MostAllocated")


# ---- the quotients ----------------------------------------------------------------------------------------------------
def _mrs_exact(req, cap):
    return [min(int(r), int(c)) * 100 // int(c) if c else 0 for r, c in zip(req, cap)]


@pytest.mark.parametrize("cap_hi,name", [(1 << 24, "cpu"), (1 << 45, "mem")])
def test_fast_mrs_exact(cap_hi, name):
    """mrs_cpu / mrs_mem equal the exact quotient on their whole domain — random pairs, every exact-integer quotient
    boundary +-1, requested in {0, cap - 1, cap, cap + 1}, small capacities and the largest — and give -1 outside it,
    where most_requested64 is still exact."""
    rng = np.random.default_rng(21 if name == "cpu" else 22)
    caps = np.concatenate([rng.integers(1, cap_hi, 30000), rng.integers(1, 4096, 5000),
                           np.array([1, 2, 3, 7, 100, 1000, 96000, cap_hi - 1, cap_hi - 2, (cap_hi - 1) // 3]),
                           np.array([g << 30 for g in (1, 3, 16, 255, 256, 1024, 4095)] +
                                    [(g << 30) + d for g in (7, 512) for d in (-1, 1, 4095)], dtype=np.int64)])
    caps = caps[caps < cap_hi]
    k = rng.integers(0, 101, len(caps))
    edge = (caps * k + 99) // 100                 # the smallest requested with quotient >= k: the boundaries
    reqs = np.concatenate([np.floor(caps * rng.random(len(caps))).astype(np.int64), edge, edge + 1, edge - 1,
                           caps, caps - 1, np.zeros_like(caps), caps + 1, caps + 5, caps * 2])
    capv = np.tile(caps, 10)
    # outside the domain: capacities at and past the bound, capacity 0, a free term below the lower bound
    out_c = np.array([cap_hi, cap_hi + 1, 2 * cap_hi, 0, 1000, 1000], dtype=np.int64)
    out_r = np.array([5, cap_hi, 3, 7, 1000 + (1 << 53), -5], dtype=np.int64)
    reqs, capv = np.concatenate([reqs, out_r]), np.concatenate([capv, out_c])
    with Engine(F.build_config(fit=MOST_ARGS), 1) as e:
        ref, oc, om = e.debug_fast_mrs(reqs, capv)
    got = oc if name == "cpu" else om
    free = capv - reqs
    lo = -(1 << 30) if name == "cpu" else -(1 << 52) + 1
    dom = (capv > 0) & (capv < cap_hi) & (free >= lo) & (free <= capv)
    assert dom.sum() > 0.8 * len(dom) and (~dom).sum() >= 5
    assert np.all(got[~dom] == -1)
    nonneg = reqs >= 0  # the reference-shaped routine on every pair, the out-of-domain ones included
    assert ref[nonneg].tolist() == _mrs_exact(reqs[nonneg], capv[nonneg])
    assert got[dom].tolist() == _mrs_exact(reqs[dom], capv[dom])


# ---- both evaluation paths ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile", sorted(C.PROFILES))
def test_eval_paths_agree(profile):
    """eval_node, eval_fast and eval_hot on every (staged pod, node) of a 300-node cluster with three rows outside the
    fast domain and one over-committed row: no mismatch."""
    cl = synth.make_cluster(300, seed=41)
    cl.nodes["allocatable"][10, abi.RES_CPU] = 1 << 24
    cl.nodes["allocatable"][20, abi.RES_MEMORY] = 1 << 45
    cl.nodes["allocatable"][30, abi.RES_CPU], cl.nodes["allocatable"][30, abi.RES_MEMORY] = (1 << 24) + 5, (1 << 45) + 4096
    cl.nodes["allocatable"][40, abi.RES_CPU], cl.nodes["allocatable"][40, abi.RES_MEMORY] = 300, 512 * C.MI
    over = np.concatenate([C.pod(0, 0)] * 5)  # 500m / 1000 MiB non-zero on a 300m / 512 MiB node
    cl.existing_pods = np.concatenate([cl.existing_pods[cl.existing_node != 40], over])
    cl.existing_node = np.concatenate([cl.existing_node[cl.existing_node != 40], np.full(5, 40, np.int32)])
    pods = np.concatenate([C.parity_queue(129, 60), C.pod(0, 0)])
    with Engine(C.parity_config(profile), cl.n) as e:
        synth.load_into(e, cl)
        e.stage(pods)
        assert e.debug_eval_paths() == 0
        _, fit, _ = e.evaluate(pods[-1])
    assert fit[40] == 100  # the over-committed row: both quotients are 100 (LeastAllocated: 0)


# ---- known answers --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", C.KNOWN, ids=lambda c: c.name)
def test_known_answers_on_the_device(c):
    cl, pods = C.known_cluster()
    k = C.KNOWN.index(c)
    with Engine(C.known_config(c), cl.n) as e:
        synth.load_into(e, cl)
        _, fit, _ = e.evaluate(pods[k])
        assert fit[k] == c.most, c.why
    if c.least is not None:
        with Engine(C.known_config(c, "LeastAllocated"), cl.n) as e:
            synth.load_into(e, cl)
            assert e.evaluate(pods[k])[1][k] == c.least, c.why
    # Engine.schedule on the case's node alone: the total is the score (Fit alone, weight 1)
    one, _ = C.known_cluster([c])
    for count in (1, 3):  # the single-pod path, and a round of the round engine (the case's pod first)
        with Engine(C.known_config(c), 1) as e:
            synth.load_into(e, one)
            node, score, _ = e.schedule(np.concatenate([pods[k]] * count))
        assert (node[0], score[0]) == (0, c.most), (count, c.why)


# ---- parity with the model ------------------------------------------------------------------------------------------
_model = {}


def _model_run(key, cfg, cl, pods, quotas=None):
    """the model's answer, computed once per input and shared (left unchanged)"""
    if key not in _model:
        res = R.schedule(cfg, cl, pods, R.MOST, quotas=quotas, batches=C.BATCHES)
        C.assert_exercises(res, cl.n, bool(cfg[0]["fit_filter"]), str(key))
        _model[key] = res
    return _model[key]


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
    bad = np.nonzero(node != want.node)[0]
    assert len(bad) == 0, f"{what}: pod {bad[0]}: node {node[bad[0]]}, the model's {want.node[bad[0]]} ({len(bad)} differ)"
    placed = want.node >= 0
    assert np.array_equal(score[placed], want.score[placed]), what
    ms = model_state(want.st)
    for name in ms:
        assert np.array_equal(state[name], ms[name]), f"{what}: {name}"
    if want.quotas is not None:
        assert np.array_equal(quotas, want.quotas), what


@pytest.mark.parametrize("depth", C.DEPTHS)
@pytest.mark.parametrize("profile", sorted(C.PROFILES))
@pytest.mark.parametrize("n_nodes", C.SIZES)
def test_parity_with_the_model(n_nodes, profile, depth):
    cl, pods = C.parity_cluster(n_nodes), C.parity_queue(n_nodes)
    want = _model_run((n_nodes, profile), C.parity_config(profile), cl, pods)
    for batch in C.BATCHES:
        cfg = C.parity_config(profile, batch_pods=batch, pipeline_depth=depth)
        _compare(_device_run(cfg, cl, pods), want, f"{n_nodes} nodes, {profile}, depth {depth}, batch {batch}")


@pytest.mark.parametrize("profile", sorted(C.PROFILES))
def test_parity_two_pod_calls(profile):
    """calls of 2 pods take the single-pod path; the rest of the queue the round engine, on the state they left"""
    cl, pods = C.parity_cluster(1100), C.parity_queue(1100)
    want = _model_run((1100, profile), C.parity_config(profile), cl, pods)
    calls = [(f, 2) for f in range(0, 60, 2)] + [(60, len(pods) - 60)]
    _compare(_device_run(C.parity_config(profile, batch_pods=38, pipeline_depth=2), cl, pods, calls), want,
             f"{profile}, 2-pod calls")


@pytest.mark.parametrize("batch,depth", [(16, 3), (38, 2), (64, 1)])
def test_parity_aux_requests(batch, depth):
    cl, pods = C.aux_inputs()
    assert (pods["requests"][:, abi.RES_EPHEMERAL] > 0).sum() > 100
    want = _model_run(("aux",), C.parity_config("fit-la-1-1"), cl, pods)
    plain = _model_run((1100, "fit-la-1-1"), C.parity_config("fit-la-1-1"), C.parity_cluster(1100), C.parity_queue(1100))
    assert not np.array_equal(want.node, plain.node)  # the ephemeral-storage requests decide some placements
    _compare(_device_run(C.parity_config("fit-la-1-1", batch_pods=batch, pipeline_depth=depth), cl, pods), want,
             f"aux requests, batch {batch}, depth {depth}")


@pytest.mark.parametrize("batch,depth", [(16, 3), (38, 2), (64, 1)])
def test_parity_with_quotas(batch, depth):
    cl, pods, quotas = C.quota_inputs()
    want = _model_run(("quota",), C.parity_config("fit-la-1-1"), cl, pods, quotas)
    rejected = sum(1 for j in range(len(pods)) if want.node[j] < 0 and pods["quota_id"][j] > 0)
    assert rejected >= 10 and (want.quotas["used"] > 0).any()
    _compare(_device_run(C.parity_config("fit-la-1-1", batch_pods=batch, pipeline_depth=depth), cl, pods, quotas=quotas),
             want, f"quotas, batch {batch}, depth {depth}")


def test_strategy_changes_placements_and_least_is_unchanged():
    """the same build, the same inputs: LeastAllocated is the oracle's answer still, MostAllocated the model's"""
    from oracle import oracle
    cl, pods = C.parity_cluster(1100), C.parity_queue(1100)
    cfg = C.parity_config("fit-la-1-1", "LeastAllocated", batch_pods=38)
    node, score, _, _ = _device_run(cfg, cl, pods)
    want_node, want_score, _ = oracle.schedule_cluster(cfg, cl, pods)
    assert np.array_equal(node, want_node) and np.array_equal(score, want_score)
    assert not np.array_equal(node, _model_run((1100, "fit-la-1-1"), C.parity_config("fit-la-1-1"), cl, pods).node)


# ---- the resolver alone -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.SCENARIOS))
def test_resolver_scenarios(name):
    """resolve_round through kg_debug_resolve on the scenarios a monotone resolver answers wrongly (n_prev 0, 1, and 1
    at batch_pods 64): out_keys and the published list are the sequential answer's."""
    s = C.SCENARIOS[name]()
    cfg = C.scenario_config(s, depth=2)
    snap = R.initial_states(cfg, s.cl)
    prev = [[(s.queue[pi:pi + 1], nd) for pi, nd in lst] for lst in s.prev]
    want, published, st = R.sequential_answer(cfg, s.cl, snap, s.queue[:s.nb], prev)
    skip = R.skip_rule_answer(cfg, s.cl, snap, s.queue[:s.nb], prev)
    assert skip != want
    with Engine(cfg, s.cl.n) as e:
        synth.load_into(e, s.cl)
        e.stage(s.queue)
        dev = e.debug_resolve(0, s.nb, s.prev)
        state = e.read_state()
    assert dev["error"] == 0 and dev["consumed"] == s.nb and dev["poison"] == 0
    assert [int(k) for k in dev["out_keys"]] == want, [R.key_node(k) for k in dev["out_keys"]]
    assert dev["list"].tolist() == published
    assert dev["slow"] == (s.nb if s.prev else s.nb - 1)  # every pod re-scores the modified rows once there are any
    ms = model_state(st)
    for col in ms:
        assert np.array_equal(state[col], ms[col]), col


# ---- nominated pods ---------------------------------------------------------------------------------------------------
def test_nominated_pods_with_most_allocated(monkeypatch):
    """schedule_staged(..., priorities) against nominated_reference composed with the MostAllocated keys: 64 nodes, 8
    entries, two of them preemptors that come through the queue."""
    cl = synth.make_cluster(64, seed=51)
    rng = np.random.default_rng(52)
    entries = C.parity_queue(129, 8)
    entries["uid"] = 900 + np.arange(8)
    e_nodes, e_prio = rng.choice(64, 8, replace=False).astype(np.int32), np.full(8, 100, np.int32)
    queue = C.parity_queue(129, 60)
    queue["uid"] = 10 + np.arange(60)
    queue[7], queue[30] = entries[2], entries[5]
    prio = rng.choice(np.array([50, 100, 150], np.int32), 60)
    cfg = C.parity_config("fit-only", batch_pods=16)
    monkeypatch.setattr(NR, "plain_keys", lambda cfg, cluster, st, pod, numa=None: R.keys(cfg, cluster, st, pod, R.MOST))
    table = NR.Table(entries, e_nodes, e_prio)
    want_node, want_score, want_st = NR.schedule(cfg, cl, queue, prio, table)
    monkeypatch.undo()
    least_node, _, _ = NR.schedule(C.parity_config("fit-only", "LeastAllocated"), cl, queue, prio,
                                   NR.Table(entries, e_nodes, e_prio))
    assert not np.array_equal(want_node, least_node) and (want_node >= 0).sum() >= 30
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


# ---- refusals -------------------------------------------------------------------------------------------------------
FIT, LA = C.FIT, C.LA
REFUSED = {
    "NodeNUMAResource": F.Profile(filter=(FIT, LA, F.NODE_NUMA_RESOURCE), score={FIT: 1, LA: 1, F.NODE_NUMA_RESOURCE: 1}),
    "DeviceShare": F.Profile(filter=(FIT, LA, F.DEVICE_SHARE), score={FIT: 1, LA: 1, F.DEVICE_SHARE: 1}),
    "Reservation": F.Profile(filter=(FIT, LA, F.RESERVATION), score={FIT: 1, LA: 1, F.RESERVATION: 1}),
    "TaintToleration": F.Profile(filter=(FIT, LA, F.TAINT_TOLERATION), score={FIT: 1, LA: 1}),
    "NodeAffinity": F.Profile(filter=(FIT, LA), score={FIT: 1, LA: 1, F.NODE_AFFINITY: 1}),
    "BalancedAllocation": F.Profile(filter=(FIT, LA), score={FIT: 1, LA: 1, F.BALANCED_ALLOCATION: 1}),
    "ImageLocality": F.Profile(filter=(FIT, LA), score={FIT: 1, LA: 1, F.IMAGE_LOCALITY: 1}),
    "PodTopologySpread": F.Profile(filter=(FIT, LA, F.POD_TOPOLOGY_SPREAD), score={FIT: 1, LA: 1}),
    "InterPodAffinity": F.Profile(filter=(FIT, LA, F.INTER_POD_AFFINITY), score={FIT: 1, LA: 1}),
}


@pytest.mark.parametrize("plugin", sorted(REFUSED))
def test_refused_combinations(plugin):
    with pytest.raises(KoordGPUError) as err:
        Engine(F.build_config(profile=REFUSED[plugin], fit=MOST_ARGS), 64)
    assert err.value.code == abi.E_UNSUPPORTED and "MostAllocated" in str(err.value)
    with Engine(F.build_config(profile=REFUSED[plugin]), 64):  # LeastAllocated: the profile runs as before
        pass


def test_refused_with_several_ranks():
    from koordinator_amd.engine import Loopback
    with Loopback(2) as g:
        with pytest.raises(KoordGPUError) as err:
            Engine(F.build_config(fit=MOST_ARGS), 64, rank=0, n_ranks=2, loopback=g)
        assert err.value.code == abi.E_UNSUPPORTED and "MostAllocated" in str(err.value)


@pytest.mark.parametrize("value", [2, -1, 7])
def test_out_of_range_strategy_is_invalid(value):
    cfg = F.build_config()
    cfg["fit_scoring_strategy"] = value
    with pytest.raises(KoordGPUError) as err:
        Engine(cfg, 8)
    assert err.value.code == abi.E_INVALID
