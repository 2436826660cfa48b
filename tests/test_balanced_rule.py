"""NodeResourcesBalancedAllocation on the round engine, without a GPU: the rule's known answers and
its float64 rounding against the committed oracle, the plain model of tests/balanced_reference.py anchored on
oracle.schedule_resv, and the two scenarios that tell the resolver's rule from the monotone one."""
import math

import numpy as np
import pytest

import balanced_cases as C
import balanced_reference as R
from koordinator_amd import abi, framework
from oracle import oracle

F = framework


# ---- the rule ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alloc,req,pod,resources,want,why", C.KNOWN, ids=[k[5].split(":")[0] for k in C.KNOWN])
def test_known_answers(alloc, req, pod, resources, want, why):
    assert C.go_balanced(alloc, req, pod, resources) == want, why
    assert oracle.balanced_score(alloc[0], alloc[1], req[0], req[1], pod[0], pod[1], resources) == want, why
    got = R.balanced_scores(np.array([alloc]), np.array([req]), pod, resources)
    assert got.tolist() == [want], why


def test_values_within_an_ulp_of_an_integer():
    """(1 − std)·100 just below, just above and exactly on an integer: int64() truncates, so the side decides the score.
    The oracle, the Python-float restatement and the model's numpy form agree on every such triple, and the sweep holds
    triples of each side."""
    alloc, req, pod = C.near_integer_triples()
    sides = [C.near_integer(a, r, p, ulps=1) for a, r, p in zip(alloc.tolist(), req.tolist(), pod.tolist())]
    assert sides.count(-1) >= 5 and sides.count(1) >= 5 and sides.count(2) >= 5, (sides.count(-1), sides.count(1))
    for a, r, p, side in zip(alloc.tolist(), req.tolist(), pod.tolist(), sides):
        want = C.go_balanced(a, r, p)
        f = [min((r[k] + p[k]) / a[k], 1.0) for k in range(2)]
        x = (1 - abs((f[0] - f[1]) / 2)) * 100.0
        if side == -1:  # just below the integer: truncation drops a whole point
            assert want == round(x) - 1 and round(x) - x <= math.ulp(x)
        elif side in (1, 2):
            assert want == round(x)
        assert oracle.balanced_score(a[0], a[1], r[0], r[1], p[0], p[1]) == want, (a, r, p)
        assert R.balanced_scores(np.array([a]), np.array([r]), p).tolist() == [want], (a, r, p)


def test_numpy_form_equals_the_oracle_on_random_rows():
    rng = np.random.default_rng(11)
    n = 3000
    alloc = np.stack([rng.integers(0, 200_000, n), rng.integers(0, 1 << 40, n)], axis=1)
    alloc[::50, 0] = 0
    alloc[25::50, 1] = 0
    req = np.stack([rng.integers(0, 250_000, n), rng.integers(0, 1 << 40, n)], axis=1)
    for resources in (1, 2, 3):
        pod = (int(rng.integers(0, 20_000)), int(rng.integers(0, 1 << 34)))
        got = R.balanced_scores(alloc, req, pod, resources)
        want = [oracle.balanced_score(int(a[0]), int(a[1]), int(r[0]), int(r[1]), pod[0], pod[1], resources)
                for a, r in zip(alloc, req)]
        assert got.tolist() == want
    assert (got == 100).sum() < n  # (the rule is not the constant)


# ---- the model is the oracle's exact pass -----------------------------------------------------------------------------
@pytest.mark.parametrize("profile", sorted(C.PROFILES))
@pytest.mark.parametrize("n_nodes", [129, 1100])
def test_model_equals_oracle_schedule_resv(n_nodes, profile):
    cfg = C.parity_config(profile)
    cl, pods = C.parity_cluster(n_nodes), C.parity_queue(n_nodes, 200)
    got = R.schedule(cfg, cl, pods)
    node, score, st, _ = R.oracle_schedule(cfg, cl, pods)
    assert np.array_equal(got.node, node)
    assert np.array_equal(got.score[node >= 0], score[node >= 0])
    assert np.array_equal(got.st["requested"], st["requested"]) and np.array_equal(got.st["nonzero"], st["nonzero"])
    # the inputs do what the parity tests rely on: most pods are placed, and Balanced moves placements
    assert (node >= 0).sum() * 2 > len(pods)
    plain = R.oracle_schedule(F.build_config(profile=C.without_balanced(profile)), cl, pods)[0]
    assert not np.array_equal(plain, node)


def test_model_equals_oracle_with_quotas():
    cl, pods, quotas = C.quota_inputs()
    pods, cfg = pods[:200], C.parity_config("fit-la-bal-1-1-1")
    got = R.schedule(cfg, cl, pods, quotas=quotas)
    node, score, st, q = R.oracle_schedule(cfg, cl, pods, quotas=quotas)
    assert np.array_equal(got.node, node) and np.array_equal(got.quotas, q)
    assert any(node[j] < 0 and pods["quota_id"][j] > 0 for j in range(len(pods)))


# ---- the two resolver scenarios ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.SCENARIOS))
def test_scenarios_tell_the_rules_apart(name):
    s = C.SCENARIOS[name]()
    cfg = C.scenario_config(s)
    snap = R.initial_states(cfg, s.cl)
    prev = [[(s.queue[pi:pi + 1], nd) for pi, nd in lst] for lst in s.prev]
    want, published, _ = R.sequential_answer(cfg, s.cl, snap, s.queue[:s.nb], prev)
    assert [R.key_node(k) for k in want] == s.want_nodes
    skip = R.skip_rule_answer(cfg, s.cl, snap, s.queue[:s.nb], prev)
    assert skip[:s.skip_differs_at] == want[:s.skip_differs_at] and skip[s.skip_differs_at] != want[s.skip_differs_at]
    # the row that wins had its key RAISED by the assume, and is not the snapshot's leader
    j = s.skip_differs_at
    w = s.want_nodes[j]
    before = int(R.keys(cfg, s.cl, snap, s.queue[j:j + 1], w, w + 1)[0])
    assert want[j] > before
    listed, _ = R.records(cfg, s.cl, snap, s.queue[j:j + 1])[0]
    assert R.key_node(listed[0]) != w
    if name == "unlisted":
        assert w not in [R.key_node(k) for k in listed]
    else:
        assert w in [R.key_node(k) for k in listed][1:]


def test_config_words():
    c = C.parity_config("la-bal-1000")[0]
    assert (c["balanced_score"], c["weight_balanced"], c["balanced_resources"], c["fit_score"]) == (1, 1000, 3, 0)
    assert "kg_debug_balanced" in abi.EXPORTED_SYMBOLS
