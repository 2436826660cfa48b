"""NodeResourcesFit RequestedToCapacityRatio on the device (kg_fit_shape_set): the shape table, the
per-resource lookup three ways, the evaluation paths, the rule's known answers, bit-exact parity of the round engine
with the plain model of tests/fit_shape_reference.py (placements, totals, node state, quotas), an anchor on the
MostAllocated engine, switching the strategy between calls, the resolver alone on the scenarios a monotone resolver gets
wrong, nominated pods, and the refusals.

Every test needs the entry points; those that schedule fail on an engine that ignores the shape (it would place by
LeastAllocated)."""
import numpy as np
import pytest

import fit_shape_cases as C
import fit_shape_reference as R
import fit_strategy_reference as S
import nominated_reference as NR
from koordinator_amd import Engine, abi, framework, synth
from koordinator_amd.abi import KoordGPUError
from resolver_model import model_state

pytestmark = pytest.mark.gpu
F = framework


def _engine(cfg, fit, n, **kw):
    return Engine(cfg, n, fit_shape=fit.shape, **kw)


# ---- the table ----------------------------------------------------------------------------------------------------------
def test_table_readback():
    """kg_fit_shape_get returns the model's table for rising, falling, peaked, one-point, 101-point and inner-point
    shapes, set one after the other on one engine; an empty shape clears it"""
    with Engine(F.build_config(), 4) as e:
        lut, active = e.fit_shape()
        assert not active and not lut.any()
        for name, shape in C.TABLE_SHAPES.items():
            e.set_fit_shape(shape)
            lut, active = e.fit_shape()
            assert active and lut.tolist() == R.table(shape), name
        e.set_fit_shape(None)
        lut, active = e.fit_shape()
        assert not active and not lut.any()
    with Engine(F.build_config(), 4, fit_shape=F.validate_fit_shape(C.PEAKED)) as e:
        assert e.fit_shape()[1] and e.fit_shape()[0].tolist() == R.table(C.PEAKED)


@pytest.mark.parametrize("cap_hi,name", [(1 << 24, "cpu"), (1 << 45, "mem")])
def test_debug_fit_shape_exact(cap_hi, name):
    """lut[u] through most_requested64, mrs_cpu and mrs_mem equals Python integers — random pairs, every quotient
    boundary +-1, requested in {0, cap - 1, cap, cap + 1, more}, small capacities and the largest — and the fast
    routines give -1 outside their domain, where the reference-shaped one is still exact; requested < 0 reads lut[0]."""
    rng = np.random.default_rng(23 if name == "cpu" else 24)
    caps = np.concatenate([rng.integers(1, cap_hi, 20000), rng.integers(1, 4096, 4000),
                           np.array([1, 2, 3, 7, 100, 1000, 96000, cap_hi - 1, cap_hi - 2, (cap_hi - 1) // 3]),
                           np.array([g << 30 for g in (1, 3, 16, 255, 256, 1024, 4095)] +
                                    [(g << 30) + d for g in (7, 512) for d in (-1, 1, 4095)], dtype=np.int64)])
    caps = caps[caps < cap_hi]
    k = rng.integers(0, 101, len(caps))
    edge = (caps * k + 99) // 100                 # the smallest requested with quotient >= k: the boundaries
    reqs = np.concatenate([np.floor(caps * rng.random(len(caps))).astype(np.int64), edge, edge + 1, edge - 1,
                           caps, caps - 1, np.zeros_like(caps), caps + 1, caps + 5, caps * 2])
    capv = np.tile(caps, 10)
    out_c = np.array([cap_hi, cap_hi + 1, 2 * cap_hi, 0, 1000, 1000], dtype=np.int64)
    out_r = np.array([5, cap_hi, 3, 7, 1000 + (1 << 53), -5], dtype=np.int64)
    reqs, capv = np.concatenate([reqs, out_r]), np.concatenate([capv, out_c])
    shape = C.FULL  # 101 points: every utilization has a value of its own neighbourhood
    lut = R.table(shape)
    with Engine(F.build_config(), 1, fit_shape=shape) as e:
        ref, oc, om = e.debug_fit_shape(reqs, capv)
    got = oc if name == "cpu" else om
    free = capv - reqs
    lo = -(1 << 30) if name == "cpu" else -(1 << 52) + 1
    dom = (capv > 0) & (capv < cap_hi) & (free >= lo) & (free <= capv)
    assert dom.sum() > 0.8 * len(dom) and (~dom).sum() >= 5
    assert np.all(got[~dom] == -1)

    def exact(r, c):
        if c == 0:
            return lut[0]  # most_requested64: capacity 0 → quotient 0
        if r < 0:
            return lut[0]  # a negative quotient reads lut[0]
        return lut[R.utilization(r, c)]
    assert ref.tolist() == [exact(int(r), int(c)) for r, c in zip(reqs, capv)]
    assert got[dom].tolist() == [exact(int(r), int(c)) for r, c in zip(reqs[dom], capv[dom])]
    assert (reqs < 0).any() and (reqs[dom] > capv[dom]).any() and (reqs[dom] == 0).any()


# ---- both evaluation paths ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(C.SHAPES))
def test_eval_paths_agree(shape):
    """eval_node, eval_fast and eval_hot on every (staged pod, node) of a 300-node cluster with three rows outside the
    fast domain and one over-committed row, under an active shape: no mismatch; the over-committed row reads lut[100]."""
    cl = synth.make_cluster(300, seed=41)
    cl.nodes["allocatable"][10, abi.RES_CPU] = 1 << 24
    cl.nodes["allocatable"][20, abi.RES_MEMORY] = 1 << 45
    cl.nodes["allocatable"][30, abi.RES_CPU], cl.nodes["allocatable"][30, abi.RES_MEMORY] = (1 << 24) + 5, (1 << 45) + 4096
    cl.nodes["allocatable"][40, abi.RES_CPU], cl.nodes["allocatable"][40, abi.RES_MEMORY] = 300, 512 * C.MI
    over = np.concatenate([C.pod(0, 0)] * 5)  # 500m / 1000 MiB non-zero on a 300m / 512 MiB node
    cl.existing_pods = np.concatenate([cl.existing_pods[cl.existing_node != 40], over])
    cl.existing_node = np.concatenate([cl.existing_node[cl.existing_node != 40], np.full(5, 40, np.int32)])
    pods = np.concatenate([C.parity_queue(129, 60), C.pod(0, 0)])
    cfg, fit = C.parity_config(shape)
    with _engine(cfg, fit, cl.n) as e:
        synth.load_into(e, cl)
        e.stage(pods)
        assert e.debug_eval_paths() == 0
        _, got, _ = e.evaluate(pods[-1])
    assert got[40] == R.table(fit.shape)[100]  # both resources read lut[100]; their mean is that value (or 0)
    st = R.initial_states(cfg, cl)
    want = R.fit_scores(fit.shape, cfg[0]["fit_resource_weights"][:2], cl.nodes["allocatable"][:, :2], st["nonzero"],
                        R.nonzero_request(cfg, pods[-1]))
    assert np.array_equal(got, want)  # kg_pods_evaluate's Fit column on every node, the rare rows included


# ---- known answers ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", C.KNOWN, ids=lambda c: c.name)
def test_known_answers_on_the_device(c):
    one, pods = C.known_cluster([c])
    for count in (1, 3):  # the single-pod path, and a round of the round engine (the case's pod first)
        cfg, fit = C.known_config(c)
        with _engine(cfg, fit, 1) as e:
            synth.load_into(e, one)
            if count == 1:
                assert e.evaluate(pods[0])[1][0] == c.want, c.why
                rows, _ = e.debug_topn(pods[0], 1)
                assert len(rows) == 1 and rows[0]["plugin"][abi.PL_FIT] == c.want and rows[0]["total"] == c.want, c.why
            node, score, _ = e.schedule(np.concatenate([pods[0]] * count))
        assert (node[0], score[0]) == (0, c.want), (count, c.why)


# ---- parity with the model ----------------------------------------------------------------------------------------------
_model = {}


def _model_run(key, cfg, fit, cl, pods, quotas=None):
    """the model's answer, computed once per input and shared (left unchanged)"""
    if key not in _model:
        res = R.schedule(cfg, cl, pods, fit.shape, quotas=quotas)
        C.assert_exercises(res, cl.n, str(key))
        _model[key] = res
    return _model[key]


def _device_run(cfg, fit, cl, pods, calls=None, quotas=None):
    with _engine(cfg, fit, cl.n) as e:
        synth.load_into(e, cl)
        if quotas is not None:
            e.set_quotas(quotas)
        e.stage(pods)
        for first, count in calls or [(0, len(pods))]:
            e.schedule_staged(first, count)
        node, score = e.fetch(0, len(pods))
        return node, score, e.read_state(), (e.read_quotas(len(quotas)) if quotas is not None else None)


def _compare(got, want, what, upto=None):
    node, score, state, quotas = got
    wn, wsc = want.node[:upto], want.score[:upto]
    bad = np.nonzero(node[:upto] != wn)[0]
    assert len(bad) == 0, f"{what}: pod {bad[0]}: node {node[bad[0]]}, the model's {wn[bad[0]]} ({len(bad)} differ)"
    placed = wn >= 0
    assert np.array_equal(score[:upto][placed], wsc[placed]), what
    ms = model_state(want.st)
    for name in ms:
        assert np.array_equal(state[name], ms[name]), f"{what}: {name}"
    if want.quotas is not None:
        assert np.array_equal(quotas, want.quotas), what


@pytest.mark.parametrize("depth", C.DEPTHS)
@pytest.mark.parametrize("shape", sorted(C.SHAPES))
@pytest.mark.parametrize("n_nodes", C.SIZES)
def test_parity_with_the_model(n_nodes, shape, depth):
    cl, pods = C.parity_cluster(n_nodes), C.parity_queue(n_nodes)
    cfg, fit = C.parity_config(shape)
    want = _model_run((n_nodes, shape), cfg, fit, cl, pods)
    for batch in C.BATCHES:
        cfg, fit = C.parity_config(shape, batch_pods=batch, pipeline_depth=depth)
        _compare(_device_run(cfg, fit, cl, pods), want, f"{n_nodes} nodes, {shape}, depth {depth}, batch {batch}")


@pytest.mark.parametrize("shape", sorted(C.SHAPES))
def test_parity_two_pod_calls(shape):
    """calls of 2 pods take the single-pod path; the rest of the queue the round engine, on the state they left"""
    cl, pods = C.parity_cluster(1100), C.parity_queue(1100)
    cfg, fit = C.parity_config(shape)
    want = _model_run((1100, shape), cfg, fit, cl, pods)
    calls = [(f, 2) for f in range(0, 60, 2)] + [(60, len(pods) - 60)]
    cfg, fit = C.parity_config(shape, batch_pods=38, pipeline_depth=2)
    _compare(_device_run(cfg, fit, cl, pods, calls), want, f"{shape}, 2-pod calls")


@pytest.mark.parametrize("batch,depth,shape", [(16, 3, "rising"), (38, 2, "peaked"), (64, 1, "falling")])
def test_parity_aux_requests(batch, depth, shape):
    cl, pods = C.aux_inputs()
    assert (pods["requests"][:, abi.RES_EPHEMERAL] > 0).sum() > 100
    cfg, fit = C.parity_config(shape)
    want = _model_run(("aux", shape), cfg, fit, cl, pods)
    plain = _model_run((1100, shape), cfg, fit, C.parity_cluster(1100), C.parity_queue(1100))
    assert not np.array_equal(want.node, plain.node)  # the ephemeral-storage requests decide some placements
    cfg, fit = C.parity_config(shape, batch_pods=batch, pipeline_depth=depth)
    _compare(_device_run(cfg, fit, cl, pods), want, f"aux requests, {shape}, batch {batch}, depth {depth}")


@pytest.mark.parametrize("batch,depth,shape", [(16, 3, "peaked"), (38, 2, "falling"), (64, 1, "rising")])
def test_parity_with_quotas(batch, depth, shape):
    cl, pods, quotas = C.quota_inputs()
    cfg, fit = C.parity_config(shape)
    want = _model_run(("quota", shape), cfg, fit, cl, pods, quotas)
    rejected = sum(1 for j in range(len(pods)) if want.node[j] < 0 and pods["quota_id"][j] > 0)
    assert rejected >= 10 and (want.quotas["used"] > 0).any()
    cfg, fit = C.parity_config(shape, batch_pods=batch, pipeline_depth=depth)
    _compare(_device_run(cfg, fit, cl, pods, quotas=quotas), want, f"quotas, {shape}, batch {batch}, depth {depth}")


# ---- an anchor that does not rest on the new model ----------------------------------------------------------------------
@pytest.mark.parametrize("n_nodes,batch", [(129, 16), (1100, 38)])
def test_identity_shape_on_one_resource_places_as_most_allocated(n_nodes, batch):
    """cpu-only weight and the identity shape: the same placements, totals and node state as an engine created with
    MostAllocated (one weighted resource: neither the rounding nor the r > 0 gate can show)"""
    cl, pods = C.parity_cluster(n_nodes), C.parity_queue(n_nodes)
    w = {"cpu": 1, "memory": 0}
    prof = C.PROFILES["fit-la-1-1"]
    most_cfg = F.build_config(fit=F.NodeResourcesFitArgs(w, "MostAllocated"), batch_pods=batch, **prof)
    fit = F.NodeResourcesFitArgs(w, C.RTCR, C.RISING)
    cfg = F.build_config(fit=fit, batch_pods=batch, **prof)
    with Engine(most_cfg, cl.n) as e:
        synth.load_into(e, cl)
        want_node, want_score, _ = e.schedule(pods)
        want_state = e.read_state()
    node, score, state, _ = _device_run(cfg, fit, cl, pods)
    assert (want_node >= 0).sum() > 100
    assert np.array_equal(node, want_node) and np.array_equal(score, want_score)
    for name in want_state:
        assert np.array_equal(state[name], want_state[name]), name


# ---- switching the strategy between calls -------------------------------------------------------------------------------
def test_switching_between_calls():
    """single pods (the per-pod pass and its cached graphs) and a staged batch (the round engine) under LeastAllocated,
    then under a shape, then another shape, then LeastAllocated again: every stretch equals the model continuing from
    the state the stretch before left.  A cached graph replayed with the earlier EvalParams would place by the earlier
    strategy."""
    cl, pods = C.parity_cluster(1100), C.parity_queue(1100, 420)
    cfg = F.build_config(batch_pods=38, pipeline_depth=2, **C.PROFILES["fit-la-1-1"])
    stretches = [(S.LEAST, None), (C.PEAKED, C.PEAKED), (C.RISING, C.RISING), (S.LEAST, None)]
    st = R.initial_states(cfg, cl)
    want_node, want_score = [], []
    for k, (model_shape, _) in enumerate(stretches):
        res = R.schedule(cfg, cl, pods[105 * k:105 * (k + 1)], model_shape, st=st)
        want_node.append(res.node)
        want_score.append(res.score)
    want_node, want_score = np.concatenate(want_node), np.concatenate(want_score)
    # the stretches differ: the queue placed by LeastAllocated alone is another answer
    least = R.schedule(cfg, cl, pods, S.LEAST)
    assert not np.array_equal(least.node, want_node) and (want_node >= 0).sum() > 200
    with Engine(cfg, cl.n) as e:
        synth.load_into(e, cl)
        e.stage(pods)
        for k, (_, shape) in enumerate(stretches):
            e.set_fit_shape(shape)
            assert e.fit_shape()[1] == (shape is not None)
            base = 105 * k
            for j in range(5):               # single-pod calls
                e.schedule_staged(base + j, 1)
            e.schedule_staged(base + 5, 2)   # a 2-pod call
            e.schedule_staged(base + 7, 98)  # the round engine
        node, score = e.fetch(0, len(pods))
        state = e.read_state()
    bad = np.nonzero(node != want_node)[0]
    assert len(bad) == 0, f"pod {bad[0]} (stretch {bad[0] // 105}): node {node[bad[0]]}, the model's {want_node[bad[0]]}"
    assert np.array_equal(score[want_node >= 0], want_score[want_node >= 0])
    ms = model_state(st)
    for name in ms:
        assert np.array_equal(state[name], ms[name]), name


# ---- the resolver alone -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.SCENARIOS))
def test_resolver_scenarios(name):
    """resolve_round through kg_debug_resolve on the scenarios where an assume raises a key by dropping a resource
    from the mean: out_keys and the published list are the sequential answer's, bit for bit."""
    s = C.SCENARIOS[name]()
    cfg, fit = C.scenario_config(s, depth=2)
    snap = R.initial_states(cfg, s.cl)
    prev = [[(s.queue[pi:pi + 1], nd) for pi, nd in lst] for lst in s.prev]
    want, published, st = R.sequential_answer(cfg, s.cl, snap, s.queue[:s.nb], prev, fit.shape)
    assert R.skip_rule_answer(cfg, s.cl, snap, s.queue[:s.nb], prev, fit.shape) != want
    with _engine(cfg, fit, s.cl.n) as e:
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


# ---- nominated pods -----------------------------------------------------------------------------------------------------
def test_nominated_pods_with_a_shape(monkeypatch):
    """schedule_staged(..., priorities) against nominated_reference composed with the shape's keys: 64 nodes, 8 entries,
    two of them preemptors that come through the queue."""
    cl = synth.make_cluster(64, seed=51)
    rng = np.random.default_rng(52)
    entries = C.parity_queue(129, 8)
    entries["uid"] = 900 + np.arange(8)
    e_nodes, e_prio = rng.choice(64, 8, replace=False).astype(np.int32), np.full(8, 100, np.int32)
    queue = C.parity_queue(129, 60)
    queue["uid"] = 10 + np.arange(60)
    queue[7], queue[30] = entries[2], entries[5]
    prio = rng.choice(np.array([50, 100, 150], np.int32), 60)
    cfg, fit = C.parity_config("peaked", batch_pods=16)
    least_node, _, _ = NR.schedule(cfg, cl, queue, prio, NR.Table(entries, e_nodes, e_prio))
    monkeypatch.setattr(NR, "plain_keys", lambda cfg, cluster, st, pod, numa=None: R.keys(cfg, cluster, st, pod, fit.shape))
    table = NR.Table(entries, e_nodes, e_prio)
    want_node, want_score, want_st = NR.schedule(cfg, cl, queue, prio, table)
    monkeypatch.undo()
    assert not np.array_equal(want_node, least_node) and (want_node >= 0).sum() >= 30
    with _engine(cfg, fit, cl.n) as e:
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


# ---- refusals -----------------------------------------------------------------------------------------------------------
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
    with Engine(F.build_config(profile=REFUSED[plugin]), 64) as e:  # LeastAllocated: the profile runs as before
        with pytest.raises(KoordGPUError) as err:
            e.set_fit_shape(C.PEAKED)
        assert err.value.code == abi.E_UNSUPPORTED and "RequestedToCapacityRatio" in str(err.value)
        assert not e.fit_shape()[1]
        e.set_fit_shape(None)  # clearing is always legal


def test_refused_with_several_ranks():
    from koordinator_amd.engine import Loopback
    with Loopback(2) as g:
        # (both ranks are created: a loopback group's first scheduling call would wait for the second)
        engines = [Engine(F.build_config(), 64, rank=r, n_ranks=2, loopback=g) for r in range(2)]
        try:
            with pytest.raises(KoordGPUError) as err:
                engines[0].set_fit_shape(C.RISING)
            assert err.value.code == abi.E_UNSUPPORTED and "several ranks" in str(err.value)
        finally:
            for e in engines:
                e.close()


def test_most_allocated_plus_a_shape_is_invalid():
    with Engine(F.build_config(fit=F.NodeResourcesFitArgs(scoring_strategy="MostAllocated")), 8) as e:
        with pytest.raises(KoordGPUError) as err:
            e.set_fit_shape(C.RISING)
        assert err.value.code == abi.E_INVALID and "MostAllocated" in str(err.value)


BAD_SHAPES = {
    "102-points": [(u, 1) for u in range(101)] + [(100, 2)],
    "utilization-below-0": [(-1, 0), (50, 5)],
    "utilization-above-100": [(0, 0), (101, 5)],
    "not-increasing": [(0, 0), (50, 5), (50, 6)],
    "decreasing": [(60, 0), (50, 5)],
    "score-below-0": [(0, -1), (100, 10)],
    "score-above-10": [(0, 0), (100, 11)],
}


def test_malformed_shapes_are_invalid_and_change_nothing():
    """every malformed shape is KG_E_INVALID; after the refused calls the engine still scores by the shape it had, and
    schedules as the model does"""
    cl, pods = C.parity_cluster(129), C.parity_queue(129, 120)
    cfg, fit = C.parity_config("peaked", batch_pods=16)
    want = R.schedule(cfg, cl, pods, fit.shape)
    with _engine(cfg, fit, cl.n) as e:
        synth.load_into(e, cl)
        for name, shape in BAD_SHAPES.items():
            with pytest.raises(KoordGPUError) as err:
                e.set_fit_shape(shape)
            assert err.value.code == abi.E_INVALID, name
            lut, active = e.fit_shape()
            assert active and lut.tolist() == R.table(fit.shape), name
        node, score, _ = e.schedule(pods)
    assert np.array_equal(node, want.node) and np.array_equal(score[want.node >= 0], want.score[want.node >= 0])


def test_without_fit_score_a_shape_has_no_effect():
    from oracle import oracle
    cl, pods = C.parity_cluster(129), C.parity_queue(129, 120)
    cfg = F.build_config(profile=F.Profile(filter=(FIT, LA), score={LA: 1}), batch_pods=16)
    want_node, want_score, _ = oracle.schedule_cluster(cfg, cl, pods)
    with Engine(cfg, cl.n, fit_shape=C.PEAKED) as e:
        assert e.fit_shape()[1]
        synth.load_into(e, cl)
        node, score, _ = e.schedule(pods)
    assert np.array_equal(node, want_node) and np.array_equal(score, want_score)
