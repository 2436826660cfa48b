"""NodeResourcesFit RequestedToCapacityRatio without a GPU: the plain model of
tests/fit_shape_reference.py against hand-derived answers, its integer and vector forms against the definition, its
anchor on the MostAllocated model, the scenarios that tell the resolver's rule from the monotone one, and the
configuration surface."""
import numpy as np
import pytest

import fit_shape_cases as C
import fit_shape_reference as R
import fit_strategy_reference as S
from koordinator_amd import abi, framework, synth

F = framework


# ---- the broken-linear function ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,p,want,why", C.RAW, ids=[f"{i}-p{c[1]}" for i, c in enumerate(C.RAW)])
def test_raw_known_answers(shape, p, want, why):
    assert R.raw(shape, p) == want, why
    assert R.table(shape)[min(max(p, 0), 100)] == want, why


def test_go_division_truncates_where_python_floors():
    assert R.go_div(-100, 3) == -33 and -100 // 3 == -34
    assert R.go_div(100, 3) == 33 and R.go_div(-99, 3) == -33 and R.go_div(0, 7) == 0


@pytest.mark.parametrize("name", sorted(C.TABLE_SHAPES))
def test_tables_stay_in_range_and_hit_their_points(name):
    shape = C.TABLE_SHAPES[name]
    lut = R.table(shape)
    assert len(lut) == 101 and all(0 <= v <= 100 for v in lut)
    for u, s in shape:
        assert lut[u] == 10 * s
    assert all(v == 10 * shape[0][1] for v in lut[:shape[0][0] + 1])
    assert all(v == 10 * shape[-1][1] for v in lut[shape[-1][0]:])


# ---- the node score ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", C.KNOWN, ids=lambda c: c.name)
def test_known_answers(c):
    cl, pods = C.known_cluster([c])
    cfg, _ = C.known_config(c)
    st = R.initial_states(cfg, cl)
    nz_pod = R.nonzero_request(cfg, pods[0])
    got = R.fit_score(c.shape, c.weights, cl.nodes["allocatable"][0, :2], st["nonzero"][0], nz_pod)
    assert got == c.want, c.why
    assert int(R.fit_scores(c.shape, c.weights, cl.nodes["allocatable"][:, :2], st["nonzero"], nz_pod)[0]) == c.want
    assert int(R.keys(cfg, cl, st, pods[0], c.shape)[0]) >> 32 == c.want  # Fit alone, weight 1: the total is the score
    if c.most is not None:
        assert S.fit_score(S.MOST, c.weights, cl.nodes["allocatable"][0, :2], st["nonzero"][0], nz_pod) == c.most, c.why


WEIGHT_PAIRS = [(1, 1), (1, 0), (0, 1), (3, 1), (2, 3), (7, 9), (1000000, 1000000), (1000000, 1), (999999, 1000000)]


@pytest.mark.parametrize("weights", WEIGHT_PAIRS, ids=lambda w: f"{w[0]}-{w[1]}")
def test_integer_rounding_equals_float_rounding(weights):
    """(2s + ws) // (2ws) == round-half-away(float(s) / float(ws)) for every reachable (s, ws): ws is the sum of the
    weights of the resources with a score > 0, s = sum r*w with r in 1..100.  (1, 1) and (1000000, 1000000) make exact
    halves at every odd r_cpu + r_mem; the pairs with 10^6 are the validated maxima."""
    wc, wm = weights
    r = np.arange(0, 101, dtype=np.int64)
    rc, rm = np.meshgrid(r, r, indexing="ij")
    s = np.where(rc > 0, rc * wc, 0) + np.where(rm > 0, rm * wm, 0)
    ws = np.where(rc > 0, wc, 0) + np.where(rm > 0, wm, 0)
    ok = ws > 0
    s, ws = s[ok], ws[ok]
    assert (s <= 100 * ws).all() and int(ws.max()) <= 2 * 10**6
    integer = (2 * s + ws) // (2 * ws)
    want = np.array([R.round_half_away(float(a) / float(b)) for a, b in zip(s.tolist(), ws.tolist())])
    assert np.array_equal(integer, want)
    if wc == wm and wc:
        assert ((2 * s) % (2 * ws) == ws).any()  # exact halves are among the cases
    # and around every half boundary of the largest weight sum: s = k*ws + ws/2 - 1, ws/2, ws/2 + 1
    big = 2 * 10**6
    for k in (0, 1, 37, 99):
        for d in (-1, 0, 1):
            sv = k * big + big // 2 + d
            assert (2 * sv + big) // (2 * big) == R.round_half_away(float(sv) / float(big)) == k + (d >= 0)


@pytest.mark.parametrize("shape", sorted(C.SHAPES))
def test_vector_form_equals_the_definition(shape):
    cl = synth.make_cluster(300, seed=41)
    cl.nodes["allocatable"][5, abi.RES_MEMORY] = 0
    cl.nodes["allocatable"][6, abi.RES_CPU] = 0
    cfg, fit = C.parity_config(shape)
    st = R.initial_states(cfg, cl)
    w = cfg[0]["fit_resource_weights"][:2]
    for pod in C.parity_queue(129, 12):
        nz = R.nonzero_request(cfg, pod)
        vec = R.fit_scores(fit.shape, w, cl.nodes["allocatable"][:, :2], st["nonzero"], nz)
        one = [R.fit_score(fit.shape, w, cl.nodes["allocatable"][i, :2], st["nonzero"][i], nz) for i in range(cl.n)]
        assert vec.tolist() == one


# ---- the anchor on the MostAllocated model ------------------------------------------------------------------------------
def _anchor_cfg(weights, strategy, shape=None):
    return F.build_config(profile=F.Profile(filter=(C.FIT, C.LA), score={C.FIT: 1, C.LA: 1}),
                          fit=F.NodeResourcesFitArgs(weights, strategy, shape))


def test_identity_shape_on_one_resource_is_most_allocated():
    """one weighted resource: s/ws is the integer r itself, so neither the rounding nor the r > 0 gate can show"""
    cl, pods = C.parity_cluster(129), C.parity_queue(129, 200)
    w = {"cpu": 1, "memory": 0}
    got = R.schedule(_anchor_cfg(w, C.RTCR, C.RISING), cl, pods, C.RISING)
    want = S.schedule(_anchor_cfg(w, "MostAllocated"), cl, pods, S.MOST)
    assert np.array_equal(got.node, want.node) and np.array_equal(got.score, want.score) and (got.node >= 0).sum() > 50


def test_identity_shape_on_two_resources_is_not():
    cl, pods = C.parity_cluster(129), C.parity_queue(129, 200)
    w = {"cpu": 1, "memory": 1}
    got = R.schedule(_anchor_cfg(w, C.RTCR, C.RISING), cl, pods, C.RISING)
    want = S.schedule(_anchor_cfg(w, "MostAllocated"), cl, pods, S.MOST)
    assert not (np.array_equal(got.node, want.node) and np.array_equal(got.score, want.score))


# ---- the resolver scenarios -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.SCENARIOS))
def test_scenario_discriminates(name):
    """the sequential answer is the hand-derived one, an assume RAISED the winner's key, and a resolver keeping the
    monotone rule answers differently at the pod the scenario names"""
    s = C.SCENARIOS[name]()
    cfg, fit = C.scenario_config(s)
    snap = R.initial_states(cfg, s.cl)
    prev = [[(s.queue[pi:pi + 1], nd) for pi, nd in lst] for lst in s.prev]
    want, published, _ = R.sequential_answer(cfg, s.cl, snap, s.queue[:s.nb], prev, fit.shape)
    assert [R.key_node(k) for k in want] == s.want_nodes and published == s.want_nodes
    skip = R.skip_rule_answer(cfg, s.cl, snap, s.queue[:s.nb], prev, fit.shape)
    assert skip[:s.skip_differs_at] == want[:s.skip_differs_at]
    assert len(skip) > s.skip_differs_at and skip[s.skip_differs_at] != want[s.skip_differs_at]
    # the last pod's winner: its key on the snapshot is BELOW its key when the pod is placed (a resource's score reached
    # 0 and left the mean), and below the best untouched candidate's
    last, w = s.queue[s.nb - 1:s.nb], s.want_nodes[-1]
    on_snap = int(R.keys(cfg, s.cl, snap, last, fit.shape, w, w + 1)[0])
    assert on_snap < want[-1] and (on_snap >> 32, want[-1] >> 32) == (50, 80)
    listed, _ = R.records(cfg, s.cl, snap, last, fit.shape)[0]
    nodes = [R.key_node(k) for k in listed]
    assert nodes[0] != w and (w not in nodes if name == "unlisted" else nodes.index(w) > 0)


# ---- configuration surface --------------------------------------------------------------------------------------------
BAD_SHAPES = {
    "empty": [],
    "102-points": [(u, 1) for u in range(101)] + [(100, 2)],
    "utilization-below-0": [(-1, 0), (50, 5)],
    "utilization-above-100": [(0, 0), (101, 5)],
    "not-increasing": [(0, 0), (50, 5), (50, 6)],
    "decreasing": [(60, 0), (50, 5)],
    "score-below-0": [(0, -1), (100, 10)],
    "score-above-10": [(0, 0), (100, 11)],
}


@pytest.mark.parametrize("name", sorted(BAD_SHAPES))
def test_malformed_shapes_raise(name):
    with pytest.raises(ValueError, match="RequestedToCapacityRatio"):
        F.build_config(fit=F.NodeResourcesFitArgs(scoring_strategy=C.RTCR, shape=BAD_SHAPES[name]))
    with pytest.raises(ValueError):
        F.validate_fit_shape(BAD_SHAPES[name])


def test_build_config_with_a_shape_leaves_the_word_zero():
    base = F.build_config()
    for name, shape in C.TABLE_SHAPES.items():
        cfg = F.build_config(fit=F.NodeResourcesFitArgs(scoring_strategy=C.RTCR, shape=shape))
        assert cfg.dtype == abi.CONFIG_DTYPE and int(cfg[0]["fit_scoring_strategy"]) == 0, name
        assert cfg.tobytes() == base.tobytes(), name  # the shape is nowhere in kg_config
    arr = F.validate_fit_shape(C.PEAKED)
    assert arr.dtype == abi.SHAPE_POINT_DTYPE and arr.dtype.itemsize == 16
    assert arr["utilization"].tolist() == [0, 60, 100] and arr["score"].tolist() == [0, 10, 0]


def test_without_a_shape_the_strategy_is_still_refused():
    with pytest.raises(ValueError, match="RequestedToCapacityRatio"):
        F.build_config(fit=F.NodeResourcesFitArgs(scoring_strategy="RequestedToCapacityRatio"))
    assert abi.STRATEGY == {"LeastAllocated": 0, "MostAllocated": 1}
    assert abi.CONFIG_DTYPE.names[-1] == "fit_scoring_strategy"
    for sym in ("kg_fit_shape_set", "kg_fit_shape_get", "kg_debug_fit_shape"):
        assert sym in abi.EXPORTED_SYMBOLS
