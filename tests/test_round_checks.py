"""The record and list checkers (tests/round_checks.py) on the model's own output — no GPU.

The GPU tests of the wide pass and the merge (tests/test_round_records.py) are only as good as these checkers.  Here
the model's records and lists pass them, at a tile-list size and at two combined sizes, on a random and on a tie-heavy
cluster; and every single mutation a subtly wrong kernel could make — a bound off by one either way, a key dropped, a
tie order swapped, a tie resolved to the wrong node, a score off by one — is rejected, by the rule that names it."""
import numpy as np
import pytest

import round_checks as C
import round_model as M
from koordinator_amd import abi, framework, synth
from oracle import oracle

KC = 64


def _keys(cfg, cl, pods):
    st = oracle.states(cl.n)
    if len(cl.existing_pods):
        oracle.add_pods(cfg, st, cl.existing_pods, cl.existing_node)
    return [oracle.node_keys(cfg, cl.nodes, cl.metrics, st, pods[j], cl.now_ns, 0, cl.n) for j in range(len(pods))]


def _record_array(top, ub, kc=KC):
    rec = np.zeros(kc + 1, dtype=np.uint64)
    rec[:len(top)] = top
    rec[kc] = ub
    return rec


@pytest.fixture(scope="module")
def cases():
    """{name: (geom, [keys per pod])}: computed once, read-only."""
    cfg = framework.build_config()
    pods = synth.make_pods(6, seed=7)
    out = {}
    for n in (16_257, 70_000):
        out[f"random-{n}"] = (M.model_geometry(n), _keys(cfg, synth.make_cluster(n, seed=n, invalid_frac=0.1), pods))
        out[f"ties-{n}"] = (M.model_geometry(n), _keys(cfg, M.tie_cluster(n), pods[:2]))
    out["random-3000"] = (M.model_geometry(3000), _keys(cfg, synth.make_cluster(3000, seed=3), pods))
    for k in out.values():
        for v in k[1]:
            v.setflags(write=False)
    return out


NAMES = ["random-3000", "random-16257", "ties-16257", "random-70000", "ties-70000"]


@pytest.mark.parametrize("name", NAMES)
def test_model_passes_its_own_checks(cases, name):
    geom, keys = cases[name]
    assert geom["combined"] == (name != "random-3000")
    for j, kv in enumerate(keys):
        lists, (top, ub) = M.round_record(kv, geom)
        assert lists.shape == (geom["n_lists"], geom["list_len"])
        C.check_lists(lists, kv, geom, f"{name} pod {j}")
        rec = _record_array(top, ub)
        C.check_record(rec, kv, KC, f"{name} pod {j}")
        C.check_record_exact(rec, (top, ub), KC, f"{name} pod {j}")
        C.check_record_exact(rec, (top, ub), KC, f"{name} pod {j}", whole=True, union=set(lists.ravel().tolist()))
        if name.startswith("ties"):
            assert ub > 0 and (kv >> np.uint64(32) == kv[0] >> np.uint64(32)).all()
            assert [C.key_node(k) for k in top[:8]] == list(range(8))  # ties go to the lowest node index


def test_vectorised_lists_equal_the_plain_model(cases):
    """tile_record (the per-tile Python model the protocol tests use) and the array model agree on a tile-list
    geometry: the same record from the same keys."""
    geom, keys = cases["random-3000"]
    for kv in keys:
        want = M.tile_record(kv, geom["tile_nodes"], geom["list_len"], KC)
        got = M.lists_record(M.tile_lists(kv, geom["tile_nodes"], geom["list_len"]), KC)
        assert got == (want[0], want[1])


def _verdict(rec, kv, model):
    """The rule that rejects `rec`: the geometry-free part first, then the exact part; None if both pass."""
    try:
        C.check_record(rec, kv, KC)
        C.check_record_exact(rec, model, KC)
    except C.CheckFailed as f:
        return f.rule
    return None


def _exact_verdict(rec, model):
    try:
        C.check_record_exact(rec, model, KC)
    except C.CheckFailed as f:
        return f.rule
    return None


def _tie_run(top):
    """(start, end) of the first run of at least two equal-score keys."""
    sc = [k >> 32 for k in top]
    for i in range(len(sc) - 1):
        if sc[i] == sc[i + 1]:
            j = i + 1
            while j + 1 < len(sc) and sc[j + 1] == sc[i]:
                j += 1
            return i, j + 1
    raise AssertionError("no tie in the record: pick another cluster")


@pytest.mark.parametrize("name", ["ties-16257", "random-70000", "ties-70000", "random-16257"])
def test_single_mutations_are_rejected_by_name(cases, name):
    geom, keys = cases[name]
    kv = keys[0]
    lists, (top, ub) = M.round_record(kv, geom)
    model = (top, ub)
    n_ge = sum(k >= ub for k in top)
    assert ub > 0 and n_ge >= 2 and len(top) == KC, "the case must leave nodes out and keep some keys above the bound"
    good = _record_array(top, ub)
    assert _verdict(good, kv, model) is None

    # the bound, one too small: always the exact part's finding; and the geometry-free part's whenever the bound is
    # the best key left out + 1 (then ub - 1 is that node's key)
    rec = good.copy()
    rec[KC] = ub - 1
    assert _exact_verdict(rec, model) == "ub-exact"
    if (kv == np.uint64(ub - 1)).any():
        assert _verdict(rec, kv, model) == "ub-bound"
    # the bound, one too large (loose): silent in a schedule — the round only stops early.  When ub is a listed key
    # (a full list's minimum) that key falls below the bound and the exact part sees the key set change as well
    rec = good.copy()
    rec[KC] = ub + 1
    assert _exact_verdict(rec, model) == "ub-exact"
    assert _verdict(rec, kv, model) == "ub-exact"

    # one listed key removed: the best one (the prefix breaks at rank 0), the last one at or above the bound (an
    # unlisted node now reaches the bound)
    for pos, rule in ((0, "prefix"), (n_ge - 1, "ub-bound")):
        rec = good.copy()
        rec[pos:KC - 1] = good[pos + 1:KC]
        rec[KC - 1] = 0
        assert _verdict(rec, kv, model) == rule, pos

    # two equal-score keys swapped
    a, b = _tie_run(top)
    rec = good.copy()
    rec[a], rec[a + 1] = good[a + 1], good[a]
    assert _verdict(rec, kv, model) == "order"

    # the lowest-index node of a tie replaced by the next node of that score that is not listed (its exact key, put
    # where the order wants it): every key is genuine and sorted, but the tie went to the wrong node
    # (a random cluster may list every node of its tied scores: the tie-heavy clusters always run this)
    score = top[a] >> 32
    listed = {C.key_node(k) for k in top}
    cand = [i for i in np.nonzero(kv >> np.uint64(32) == np.uint64(score))[0].tolist()
            if i not in listed and i > C.key_node(top[a]) and int(kv[i]) != 0]
    assert cand or name.startswith("random"), "no unlisted node at the tie's score"
    if cand and a < n_ge:
        new = sorted([k for i, k in enumerate(top) if i != a] + [int(kv[cand[0]])], reverse=True)
        assert _verdict(_record_array(new, ub), kv, model) == "prefix"
    else:
        assert name.startswith("random")

    # a key whose score is off by one (still in order): not the key of its node
    rec = good.copy()
    rec[0] = good[0] + np.uint64(1 << 32)
    assert _verdict(rec, kv, model) == "key-exact"
    rec = good.copy()
    rec[KC - 1] = good[KC - 1] - np.uint64(1 << 32)
    assert _verdict(rec, kv, model) in ("key-exact",)


def test_list_mutations_are_rejected_by_name(cases):
    for name in ("random-3000", "random-70000"):
        geom, keys = cases[name]
        kv = keys[0]
        lists = M.round_lists(kv, geom)
        full = np.nonzero((lists != 0).all(axis=1))[0]
        assert len(full), "the case needs a full list"
        l = int(full[0])

        def rule(mut):
            try:
                C.check_lists(mut, kv, geom)
            except C.CheckFailed as f:
                return f.rule
            return None

        assert rule(lists) is None
        m = lists.copy()
        m[l, 0], m[l, 1] = lists[l, 1], lists[l, 0]
        assert rule(m) == "list-order"
        m = lists.copy()
        m[l, 2] = 0
        assert rule(m) == "list-zeros"
        m = lists.copy()
        m[l, -1] = 0  # a key missing, the zero at the tail
        assert rule(m) == "list-set"
        m = lists.copy()
        m[l, 3] += np.uint64(1 << 32)
        assert rule(m) == "list-set"
        m = lists.copy()[:, ::-1]  # tile order where group order is due and the reverse
        assert rule(np.ascontiguousarray(m)) in ("list-order", "list-zeros")
