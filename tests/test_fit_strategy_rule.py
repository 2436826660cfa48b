"""NodeResourcesFit ScoringStrategy MostAllocated, without a GPU: the rule's hand-derived answers, the
model's plumbing against the oracle, the three scenarios that tell the resolver's two rules apart, and the configuration
surface."""
import numpy as np
import pytest

import fit_strategy_cases as C
import fit_strategy_reference as R
from koordinator_amd import abi, framework, synth
from oracle import oracle

F = framework


def _row(cfg, cl, k):
    st = R.initial_states(cfg, cl)
    return cl.nodes["allocatable"][k, :2], st["nonzero"][k]


@pytest.mark.parametrize("c", C.KNOWN, ids=lambda c: c.name)
def test_known_answers(c):
    cl, pods = C.known_cluster()
    k = C.KNOWN.index(c)
    cfg = C.known_config(c)
    alloc, nz = _row(cfg, cl, k)
    nzp = R.nonzero_request(cfg, pods[k])
    assert R.fit_score(R.MOST, c.weights, alloc, nz, nzp) == c.most, c.why
    if c.least is not None:
        assert R.fit_score(R.LEAST, c.weights, alloc, nz, nzp) == c.least, c.why
    # the vector form the model schedules with is the same function
    st = R.initial_states(cfg, cl)
    for s in (R.MOST, R.LEAST):
        vec = R.fit_scores(s, c.weights, cl.nodes["allocatable"][:, :2], st["nonzero"], nzp)
        one = [R.fit_score(s, c.weights, cl.nodes["allocatable"][i, :2], st["nonzero"][i], nzp) for i in range(cl.n)]
        assert vec.tolist() == one
    # ... and the LeastAllocated form is the oracle's Fit score
    least_cfg = C.known_config(c, "LeastAllocated")
    got = oracle.fit_score(least_cfg, cl.nodes[k:k + 1], st[k:k + 1], pods[k])
    assert got == R.fit_score(R.LEAST, c.weights, alloc, nz, nzp)


def test_known_answers_through_the_model_keys():
    cl, pods = C.known_cluster()
    for k, c in enumerate(C.KNOWN):
        cfg = C.known_config(c)
        kv = R.keys(cfg, cl, R.initial_states(cfg, cl), pods[k], R.MOST)
        assert int(kv[k]) == R.make_key(c.most, k), (c.name, hex(int(kv[k])))


def test_zero_request_pod_nonzero_request():
    cfg = F.build_config()
    assert R.nonzero_request(cfg, C.pod(0, 0)) == (100, 200 * C.MI)
    assert R.nonzero_request(cfg, C.pod(250, 0)) == (250, 200 * C.MI)


def test_vector_scores_equal_integer_scores_on_a_synth_cluster():
    cl = synth.make_cluster(200, seed=5)
    pods = synth.make_pods(8, seed=6)
    cfg = F.build_config()
    st = R.initial_states(cfg, cl)
    for w in ((1, 1), (3, 1), (0, 2)):
        for j in range(len(pods)):
            nzp = R.nonzero_request(cfg, pods[j])
            for s in (R.MOST, R.LEAST):
                vec = R.fit_scores(s, w, cl.nodes["allocatable"][:, :2], st["nonzero"], nzp)
                one = [R.fit_score(s, w, cl.nodes["allocatable"][i, :2], st["nonzero"][i], nzp) for i in range(cl.n)]
                assert vec.tolist() == one


@pytest.mark.parametrize("profile", [None, F.Profile(filter=(C.FIT,), score={C.FIT: 3}),
                                     F.Profile(filter=(C.LA,), score={C.FIT: 1, C.LA: 2})],
                         ids=["default", "fit-only", "no-fit-filter"])
def test_least_allocated_model_is_the_oracle(profile):
    """strategy = LeastAllocated: the model (Filters + LoadAware from the oracle, Fit score in Python) places as
    oracle.schedule does — the model's own plumbing is right."""
    cl = synth.make_cluster(64, seed=21)
    pods = synth.make_pods(300, seed=22)
    cfg = F.build_config(profile=profile)
    want_node, want_score, want_st = oracle.schedule_cluster(cfg, cl, pods)
    got = R.schedule(cfg, cl, pods, R.LEAST)
    assert np.array_equal(got.node, want_node) and np.array_equal(got.score[got.node >= 0], want_score[want_node >= 0])
    for f in want_st.dtype.names:
        assert np.array_equal(got.st[f], want_st[f]), f
    assert (want_node >= 0).sum() > 100


def test_most_allocated_differs_from_least():
    cl = synth.make_cluster(64, seed=21)
    pods = synth.make_pods(100, seed=22)
    cfg = F.build_config()
    assert not np.array_equal(R.schedule(cfg, cl, pods, R.MOST).node, R.schedule(cfg, cl, pods, R.LEAST).node)


@pytest.mark.parametrize("name", sorted(C.SCENARIOS))
def test_scenario_discriminates(name):
    """The sequential answer is the hand-derived one, and a resolver keeping the monotone rule would answer otherwise."""
    s = C.SCENARIOS[name]()
    cfg = C.scenario_config(s)
    snap = R.initial_states(cfg, s.cl)
    prev = [[(s.queue[pi:pi + 1], nd) for pi, nd in lst] for lst in s.prev]
    want, published, _ = R.sequential_answer(cfg, s.cl, snap, s.queue[:s.nb], prev)
    assert [R.key_node(k) for k in want] == s.want_nodes
    skip = R.skip_rule_answer(cfg, s.cl, snap, s.queue[:s.nb], prev)
    j = s.skip_differs_at
    assert skip[:j] == want[:j] and len(skip) > j and skip[j] != want[j], (name, skip, want)
    if name == "a":  # the top listed candidate is the untouched fullest node; the touched node scores higher
        recs = R.records(cfg, s.cl, snap, s.queue[:s.nb], R.MOST)
        assert R.key_node(recs[1][0][0]) == 3 and R.key_node(skip[1]) == 3 and want[1] >> 32 == 96
    if name == "b":  # the raised node is in no record
        recs = R.records(cfg, s.cl, snap, s.queue[:s.nb], R.MOST)
        assert 70 not in [R.key_node(k) for k in recs[0][0]] and len(recs[0][0]) == R.KC
    if name == "c":  # 70 distinct touched nodes; the winner's slot is past the first bank, its key not among the probed
        touched = [nd for lst in s.prev for _, nd in lst] + published[:6]
        assert len(set(touched)) == 70 and touched.index(65) >= R.BANK
        recs = R.records(cfg, s.cl, snap, s.queue[:s.nb], R.MOST)
        assert 65 not in [R.key_node(k) for k in recs[6][0][:R.PROBE]]
        assert R.key_node(skip[6]) == 0


def test_build_config_maps_the_strategy():
    assert int(F.build_config()[0]["fit_scoring_strategy"]) == abi.STRATEGY["LeastAllocated"] == 0
    cfg = F.build_config(fit=F.NodeResourcesFitArgs(scoring_strategy="MostAllocated"))
    assert int(cfg[0]["fit_scoring_strategy"]) == abi.STRATEGY["MostAllocated"] == 1
    assert F.NodeResourcesFitArgs().scoring_strategy == "LeastAllocated"
    with pytest.raises(ValueError, match="RequestedToCapacityRatio"):
        F.build_config(fit=F.NodeResourcesFitArgs(scoring_strategy="RequestedToCapacityRatio"))


def test_config_struct_unchanged():
    """the strategy took the reserved word: same size, same offset, the last word of kg_config; ABI 18"""
    names = abi.CONFIG_DTYPE.names
    assert names[-1] == "fit_scoring_strategy" and "reserved" not in names
    off = abi.CONFIG_DTYPE.fields["fit_scoring_strategy"][1]
    assert off == abi.CONFIG_DTYPE.itemsize - 8
    assert abi.CONFIG_DTYPE.fields["ds_scoring_weights_x"][1] + 16 == off
    assert abi.ABI_VERSION == 18
    lib = abi.load_library()
    assert lib.kg_abi_version() == 18
