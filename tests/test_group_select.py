"""eval_round's tile-group select: one top-kRG select per (pod, tile group) over the values the block
staged in LDS, instead of a top-kR select per tile and a combine.  The lists must be what the tile lists' combine gave:
the model (tests/round_model.py) still builds them from tile lists, and the first test checks on the CPU that this is
the group's own top-kRG at the shapes used here.

The cases are the smallest at which the new path can go wrong: 16,773 nodes = 132 tiles, so the last block holds 4 of
its 8 tiles (its other waves stage zeros) and the last tile 5 nodes; a last pod group shorter than the others; a wave
selecting two pods; one pod; a pod group too large to stage, which takes the tile-select + combine path.  Geometry comes
from the device's out_geom."""
import numpy as np
import pytest

import round_checks as C
import round_model as M
import test_round_records as R
from koordinator_amd import Engine, abi, synth
from oracle import oracle

N = 16_773


def _group_top(keys, geom):
    """uint64[n_groups, list_len]: each tile group's list_len largest keys, descending — straight from the key vector."""
    span = geom["tile_nodes"] * geom["group_tiles"]
    ng = -(-len(keys) // span)
    k = np.zeros(ng * span, dtype=np.uint64)
    k[:len(keys)] = keys
    return np.ascontiguousarray(np.sort(k.reshape(ng, span), axis=1)[:, ::-1][:, :geom["list_len"]])


@pytest.mark.parametrize("n", [N, 16_257, 16_384 + 1_024, 1_024 * 17 - 1])
@pytest.mark.parametrize("bits", [8, 24])
def test_model_group_lists_are_the_groups_own_top(n, bits):
    """round_model.round_lists (top of the tile lists' union) == the group's top, ties and sparse groups included."""
    geom = M.model_geometry(n, score_bits=bits)
    assert geom["combined"] == 1
    rng = np.random.default_rng(n + bits)
    smax = (1 << bits) - 1
    for name in ("random", "ties", "sparse", "one-group-ties"):
        score = rng.integers(0, smax + 1, n)
        if name == "ties":
            score = smax - rng.integers(0, 3, n)
        if name == "one-group-ties":
            score[2_048:3_072] = smax // 2
        keys = (score.astype(np.uint64) << np.uint64(32)) | (np.uint64(C.M32) - np.arange(n, dtype=np.uint64))
        keys[rng.random(n) < (0.995 if name == "sparse" else 0.1)] = 0
        got = M.round_lists(keys, geom)
        np.testing.assert_array_equal(got, _group_top(keys, geom), err_msg=f"{n} nodes, {bits} bits, {name}")
        C.check_lists(got, keys, geom, name)


def _run(table, shape, weights):
    """One queue (the make_pods mix, pods with ephemeral-storage / scalar requests, pods few nodes take, one no node
    takes) read back round by round at N nodes.  → (geom, [(pod, oracle keys)])."""
    batch, ppw = shape
    cfg = R._cfg(*weights, batch=batch, ppw=ppw)
    cl = R._cluster(N, table, seed=N + 12)
    warm = synth.make_pods(150, seed=N + 13)
    on, _, st = oracle.schedule_cluster(cfg, cl, warm, n_threads=16)
    with Engine(cfg, cl.n) as e:
        synth.load_into(e, cl)
        gn, _, _ = e.schedule(warm)
        np.testing.assert_array_equal(gn, on)
        e.stage(synth.make_pods(1, seed=1))
        kc = e.debug_round_records(0, 1)[0]["kc"]
        # 38 pods: a whole round of the bench's batch, its last pod group 6 pods at 8 (and at 12 of 30) per wave
        pods, _, i_nowhere = R._probe_pods(cfg, cl, st, kc, 8 if batch == 1 else 31, N + 14)
        assert batch == 1 or len(pods) == 38
        assert (pods["requests"][:, abi.RES_EPHEMERAL] > 0).any() and (pods["requests"][:, abi.RES_BATCH_CPU] > 0).any()
        e.stage(pods)
        out = []
        for first in range(0, len(pods), batch):
            geom, lists, recs = e.debug_round_records(first, min(batch, len(pods) - first))
            out += [(first + j, lists[j], recs[j]) for j in range(len(recs))]
    print(f"geometry at {N} nodes ({table}, batch {batch}, {ppw} pods per wave): {geom}")
    assert geom["combined"] == 1 and geom["n_lists"] == -(-N // (geom["tile_nodes"] * geom["group_tiles"]))
    assert N % geom["tile_nodes"] == 5 and (-(-N // geom["tile_nodes"])) % geom["group_tiles"] == 4
    checked, full, short = [], False, False
    for j, lists, rec in out:
        what = f"{N} nodes, {table}, batch {batch}, {ppw} pods per wave, pod {j}"
        kv = oracle.node_keys(cfg, cl.nodes, cl.metrics, st, pods[j], cl.now_ns, 0, cl.n)
        C.check_lists(lists, kv, geom, what)
        np.testing.assert_array_equal(lists, _group_top(kv, geom), err_msg=what)
        mlists, model = M.round_record(kv, geom)
        C.check_record_exact(rec, model, geom["kc"], what, union=set(mlists.ravel().tolist()))
        if j != i_nowhere:
            full |= bool((lists != 0).all(axis=1).any())
            short |= bool((lists == 0).any())
        checked.append((j, kv))
    assert not np.count_nonzero(out[i_nowhere][1])
    assert full and short  # a full group list and one that is not, among the pods some node takes
    return geom, checked


@pytest.mark.gpu
@pytest.mark.parametrize("table", ["ties", "random", "rare"])
def test_group_lists_tables(table):
    geom, checked = _run(table, (38, 8), (1, 1))
    assert geom["score_bits"] == 8
    if table == "ties":  # more holders of a group's top score than a list takes, in several of its tiles
        span, ll = geom["tile_nodes"] * geom["group_tiles"], geom["list_len"]
        spread = 0
        for _, kv in checked:
            sc = np.where(kv != 0, (kv >> np.uint64(32)).astype(np.int64), -1)
            for g in range(0, N - span, span):
                top = np.nonzero((sc[g:g + span] == sc[g:g + span].max()) & (sc[g:g + span] >= 0))[0]
                spread += len(top) > ll and len(set((top // geom["tile_nodes"]).tolist())) > 1
        assert spread


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(30, 12), (1, 1), (64, 32)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_group_lists_shapes(shape):
    """(30, 12): a wave selects two pods and the last pod group holds 6; (1, 1); (64, 32): 128 KiB of values, past what
    a block stages, so the tile lists are combined as before — the same lists either way."""
    _run("random", shape, (3, 11))
    if shape == (30, 12):
        _run("ties", shape, (1, 1))


@pytest.mark.gpu
def test_group_lists_wide_scores():
    """Weights (50,000, 50,000): score_bits 24, values past 16 bits, the full bisection's range."""
    geom, checked = _run("random", (38, 8), (50_000, 50_000))
    assert geom["score_bits"] == 24
    assert max(int(kv.max() >> np.uint64(32)) for _, kv in checked) >= 1 << 16
