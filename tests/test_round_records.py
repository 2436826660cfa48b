"""The round engine's wide pass and merge, kernel by kernel, against the model (the record invariant).

The end-to-end parity tests see only the branches their inputs reach.  These read back what eval_round and the merge
kernels write (kg_debug_round_records, kg_debug_merge) and check it against oracle.node_keys and tests/round_model.py,
so a fault shows as "list 17 of pod 3 at 131,073 nodes", not as a placement that differs:
  * the merge kernels on synthetic lists: every list-count bucket of the per-wavefront merge, every chunk of the
    per-block merge, the histogram and the radix selection, narrow and wide scores, tie runs cut at every 64-list and
    256-list boundary;
  * the wide pass and the merge on real tables at the node counts where the geometry changes.
The checkers themselves are tested on the CPU (tests/test_round_checks.py).  Geometry comes from the device's
out_geom; no expected value does."""
import numpy as np
import pytest

import round_checks as C
import round_model as M
from koordinator_amd import Engine, abi, framework, synth
from koordinator_amd.abi import KoordGPUError
from oracle import oracle

pytestmark = pytest.mark.gpu

FIT, LA = framework.NODE_RESOURCES_FIT, framework.LOAD_AWARE
GI = 1 << 30
# Fit + LoadAware weights by the score_bits they give (max total = 100 · the sum; score_bits = bits to hold it)
WEIGHTS = {8: (1, 1), 10: (3, 4), 11: (3, 8), 13: (40, 41), 14: (41, 41), 24: (50_000, 50_000)}


def _cfg(wf, wl, batch=32, ppw=8):
    return framework.build_config(profile=framework.Profile(score={FIT: wf, LA: wl}), batch_pods=batch,
                                  pods_per_wave=ppw)


def _wave_bucket(n_lists):
    """Lists per lane of the per-wavefront merge for a list count (64 lanes)."""
    return 1 if n_lists <= 64 else 2 if n_lists <= 128 else 4 if n_lists <= 256 else 8


# ---------------------------------------------------------------------------------------------------
# 3a: the merge kernels on synthetic lists
# ---------------------------------------------------------------------------------------------------
SPAN = 16  # nodes a synthetic list draws from: list l holds nodes of [l·SPAN, (l + 1)·SPAN), below list l + 1's
N_WAVE = (1, 2, 8, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512)
N_BLOCK = N_WAVE + (513, 769, 1024)
N_RANK = (1, 2, 8, 128)


def _layout(score, node, order):
    """uint64[nl, ll] lists from score[nl, ll] (-1 = no key) and node[nl, ll]: 'tile' = ascending node index, 'group'
    = descending key; zeros at the tail."""
    key = (score.astype(np.uint64) << np.uint64(32)) | (np.uint64(C.M32) - node.astype(np.uint64))
    key[score < 0] = 0
    if order == "group":
        return np.ascontiguousarray(np.sort(key, axis=1)[:, ::-1])
    nd = np.where(score < 0, np.int64(1) << 40, node)
    return np.take_along_axis(key, np.argsort(nd, axis=1, kind="stable"), axis=1)


def _cases(rng, nl, ll, kc, smax):
    """[(name, score[nl, ll], node[nl, ll])]: the patterns of one (score range, list count)."""
    base = (np.arange(nl, dtype=np.int64) * SPAN)[:, None]

    def nodes():
        return base + rng.permuted(np.tile(np.arange(SPAN, dtype=np.int64), (nl, 1)), axis=1)[:, :ll]

    def sparse(lo, hi, cmin=0, cmax=None):
        cnt = rng.integers(cmin, (ll - 1 if cmax is None else cmax) + 1, nl)
        sc = rng.integers(lo, hi + 1, (nl, ll))
        sc[np.arange(ll)[None, :] >= cnt[:, None]] = -1
        return sc

    out = [("sparse", sparse(0, smax), nodes()),
           ("empty", np.full((nl, ll), -1, dtype=np.int64), nodes()),
           ("one-score-full", np.full((nl, ll), smax // 3, dtype=np.int64), nodes())]
    # scores 0 and the largest together, among enough keys that the selection runs
    sc = sparse(0, smax, cmin=ll // 2)
    u = rng.random((nl, ll))
    sc[(sc >= 0) & (u < 0.2)] = 0
    sc[(sc >= 0) & (u > 0.8)] = smax
    sc[0, 0], sc[nl - 1, 0] = 0, smax
    out.append(("extremes", sc, nodes()))
    # one full list whose minimum lies above most other keys, a few keys above it
    sc = sparse(0, smax // 2)
    j = int(rng.integers(0, nl))
    sc[j] = rng.integers(smax // 2 + 1, smax, ll)
    for _ in range(3):
        l = int(rng.integers(0, nl))
        if l != j:
            sc[l, 0] = smax
    out.append(("one-full-list", sc, nodes()))
    # totals of kc - 1, kc, kc + 1 keys: no list full where the lists can hold them so
    for total in (kc - 1, kc, kc + 1):
        cols = ll - 1 if nl * (ll - 1) >= total else ll
        if nl * cols < total:
            continue
        sc = np.full((nl, ll), -1, dtype=np.int64)
        slot = rng.permutation(nl * cols)[:total]
        sc[slot // cols, slot % cols] = rng.integers(0, smax + 1, total)
        out.append((f"total-{total}", sc, nodes()))
    # a few keys above tau, and a run of keys at tau that straddles a 64-list boundary b (every b, and the lists' two
    # ends), more of them than the record can take: `need` cuts the run in its middle
    tau = max(1, smax // 2)
    for b in sorted({0, nl} | set(range(64, nl, 64))):
        lo = max(0, min(b - 8, nl - 16))  # 16 lists around b: 80 to 16·(ll - 1) ties, the cut falls past b
        ties = [l for l in range(lo, lo + 16) if l < nl]
        sc = sparse(0, tau - 1) if tau > 1 else np.full((nl, ll), -1, dtype=np.int64)
        sc[ties] = -1
        for l in ties:
            sc[l, :int(rng.integers(ll - 3, ll))] = tau  # 5 .. ll - 1 ties: the list is not full
        above = rng.permutation(nl)[:int(rng.integers(0, 9))]
        sc[above, ll - 1] = rng.integers(tau + 1, smax + 1, len(above)) if smax > tau else tau
        for l in above:  # an above-tau key must not fill a tie list
            if (sc[l] >= 0).all():
                sc[l, ll - 2] = -1
        out.append((f"ties-at-{b}", sc, nodes()))
    return out


@pytest.fixture(scope="module", params=[8, 10, 11, 14, 24], ids=lambda b: f"bits{b}")
def merge_engine(request):
    """(engine of 1,024 nodes, its geometry) for one score width.  The geometry — kC, the list length, score_bits —
    is read from the device through one round over one staged pod."""
    wf, wl = WEIGHTS[request.param]
    cl = synth.make_cluster(1024, seed=5)
    with Engine(_cfg(wf, wl), cl.n) as e:
        synth.load_into(e, cl)
        e.stage(synth.make_pods(1, seed=6))
        geom, _, _ = e.debug_round_records(0, 1)
        assert geom["score_bits"] == request.param
        yield e, geom


@pytest.mark.parametrize("variant", [0, 1], ids=["wave", "block"])
@pytest.mark.parametrize("order", ["tile", "group"])
def test_merge_synthetic_lists(merge_engine, variant, order):
    e, geom = merge_engine
    kc, ll, smax = geom["kc"], geom["list_len"], (1 << geom["score_bits"]) - 1
    rng = np.random.default_rng(1000 * geom["score_bits"] + 10 * variant + (order == "group"))
    ran = set()
    for nl in (N_WAVE if variant == 0 else N_BLOCK):
        cases = _cases(rng, nl, ll, kc, smax)
        lists = np.stack([_layout(sc, nd, order) for _, sc, nd in cases])
        for li in lists:
            assert len(np.unique(li[li != 0])) == (li != 0).sum()  # the contract: a pod's keys are unique
        recs = e.debug_merge(variant, lists, kc)
        for (name, _, _), li, rec in zip(cases, lists, recs):
            what = f"variant {variant} {order} order, {nl} lists, score_bits {geom['score_bits']}, {name}"
            model = M.lists_record(li, kc)
            C.check_record_exact(rec, model, kc, what, whole=(variant == 1), union=set(li.ravel().tolist()))
            if name == "one-score-full" and variant == 1 and nl * ll >= kc:
                want = np.sort(C.M32 - (li.ravel() & np.uint64(C.M32)).astype(np.int64))[:kc]
                assert [C.key_node(k) for k in rec[:kc]] == want.tolist(), what  # the kc lowest node indices
            if name.startswith("ties-at") and nl >= 16:
                tau = max(1, smax // 2)
                n_tau = int(((li != 0) & ((li >> np.uint64(32)) == np.uint64(tau))).sum())
                assert n_tau > kc > sum(k >> 32 > tau for k in model[0]), what  # the run is cut in its middle
        ran.add(_wave_bucket(nl) if variant == 0 else (nl - 1) // 256)
    assert ran == ({1, 2, 4, 8} if variant == 0 else {0, 1, 2, 3})  # every L of merge_wave / chunk of merge_round


def test_merge_synthetic_rank_records(merge_engine):
    """merge_round<true>: records of several ranks (keys descending, each rank a contiguous shard, its own ub)."""
    e, geom = merge_engine
    kc, smax = geom["kc"], (1 << geom["score_bits"]) - 1
    rng = np.random.default_rng(77 + geom["score_bits"])
    stride = 128
    for nr in N_RANK:
        cases = []
        for name in ("sparse", "full", "one-score", "empty", "ub-only"):
            recs = np.zeros((nr, stride), dtype=np.uint64)
            for r in range(nr):
                m = {"sparse": int(rng.integers(0, kc)), "full": kc, "one-score": kc, "empty": 0, "ub-only": 3}[name]
                nodes = r * 4096 + rng.permutation(4096)[:m]
                sc = np.full(m, smax // 3) if name == "one-score" else rng.integers(0, smax + 1, m)
                keys = np.sort(np.array([C.make_key(s, n) for s, n in zip(sc, nodes)], dtype=np.uint64))[::-1]
                recs[r, :m] = keys
                if name == "ub-only" or (m == kc and rng.random() < 0.7):  # a rank that left nodes out
                    recs[r, kc] = C.make_key(int(rng.integers(0, smax + 1)), r * 4096 + 5000)
            cases.append((name, recs))
        got = e.debug_merge(2, np.stack([c for _, c in cases]), kc)
        for (name, recs), rec in zip(cases, got):
            what = f"rank records, {nr} ranks, score_bits {geom['score_bits']}, {name}"
            union = set(recs[:, :kc].ravel().tolist())
            C.check_record_exact(rec, M.rank_records(recs, kc), kc, what, whole=True, union=union)


def test_merge_hook_refuses_bad_input(merge_engine):
    """Checked on the host, no launch: a score outside the engine's range (the histogram is indexed by it), a list
    count past the variant's capacity, a list length no variant is compiled for."""
    e, geom = merge_engine
    kc, ll = geom["kc"], geom["list_len"]
    ok = np.zeros((1, 4, ll), dtype=np.uint64)
    ok[0, 0, 0] = C.make_key((1 << geom["score_bits"]) - 1, 3)
    for v in (0, 1):
        assert e.debug_merge(v, ok, kc)[0, 0] == ok[0, 0, 0]
    bad = ok.copy()
    bad[0, 3, 0] = C.make_key(1 << geom["score_bits"], 900)
    rank_bad = np.zeros((1, 2, 128), dtype=np.uint64)
    rank_bad[0, 1, 0] = bad[0, 3, 0]
    for v, arr in ((0, bad), (1, bad), (2, rank_bad),
                   (0, np.zeros((1, 513, ll), dtype=np.uint64)), (1, np.zeros((1, 1025, ll), dtype=np.uint64)),
                   (2, np.zeros((1, 129, 128), dtype=np.uint64)), (0, np.zeros((1, 4, 2 * ll), dtype=np.uint64)),
                   (1, np.zeros((1, 4, ll + 1), dtype=np.uint64)), (2, np.zeros((1, 4, ll), dtype=np.uint64)),
                   (3, ok)):
        with pytest.raises(KoordGPUError) as err:
            e.debug_merge(v, arr, kc)
        assert err.value.code == abi.E_INVALID, (v, arr.shape)


# ---------------------------------------------------------------------------------------------------
# 3b: the wide pass and the merge on real tables
# ---------------------------------------------------------------------------------------------------
SHAPES = ((1, 1), (33, 5), (64, 8))
WEIGHT_AXIS = ((1, 1), (3, 11), (41, 41), (40, 41))
# (nodes, combined lists, lists per lane of the merge) — the edges of the geometry
SIZES = ((1, 0, 1), (127, 0, 1), (129, 0, 1), (1_025, 0, 1), (16_256, 0, 2), (16_257, 1, 1), (65_537, 1, 2),
         (131_073, 1, 4))
TABLES = ("random", "ties", "rare")


def _real_cases():
    out, k = [], {0: 0, 1: 0}
    for n, comb, lanes in SIZES:
        for table in TABLES:
            i = k[comb]
            k[comb] += 1
            # the shape shifts by one per size, so no table keeps one shape, and every shape and every weight pair
            # comes up on either side of the combine threshold
            out.append(pytest.param(n, comb, lanes, table, SHAPES[(i + i // 3) % 3], WEIGHT_AXIS[i % 4],
                                    id=f"{n}-{table}"))
    out.append(pytest.param(262_145, 1, 8, "random", SHAPES[1], WEIGHT_AXIS[2], id="262145-random"))
    return out


def _cluster(n, table, seed):
    if table == "ties":
        cl = M.tie_cluster(n)
        big = np.arange(0, n, max(1, n // 9))[:9]  # nine larger nodes: the only ones a huge pod fits
        cl.nodes["allocatable"][big, abi.RES_CPU] = 64_000
        cl.nodes["allocatable"][big, abi.RES_MEMORY] = 256 * GI
        return cl
    cl = synth.make_cluster(n, seed=seed, invalid_frac=0.1 if n > 1 else 0.0)
    if table == "rare":  # rows outside the fast path's exact domain (as test_eval_paths_agree builds them)
        cl.nodes["raw_allocatable"][::4, :2] = cl.nodes["allocatable"][::4, :2] // 2
        cl.nodes["raw_allocatable_present"][::4, :2] = 1
        cl.nodes["flags"][::4] |= abi.NODE_HAS_RAW_ALLOCATABLE
        cl.nodes["allocatable"][5::17, abi.RES_MEMORY] = 0
    if n > 16:  # ephemeral storage on most nodes, for the pods that ask for it
        rng = np.random.default_rng(seed + 1)
        cl.nodes["allocatable"][:, abi.RES_EPHEMERAL] = np.where(rng.random(n) < 0.7, rng.choice([100, 200, 400], n) * GI, 0)
    return cl


def _probe_pods(cfg, cl, st, kc, n_mix, seed):
    """The round's queue: the make_pods mix; pods asking for ephemeral storage / a scalar resource; pods so large that
    fewer than kc nodes take them; pods that fit nowhere.  → (pods, index of the first 'few' pod, of the first
    'nowhere' pod)."""
    mix = synth.make_pods(n_mix, seed=seed)
    aux = synth.make_pods(4, seed=seed + 1)
    aux["requests"][:2, abi.RES_EPHEMERAL] = (50 * GI, 150 * GI)
    aux["requests"][2, abi.RES_BATCH_CPU] = 1000
    aux["requests"][3, abi.RES_EPHEMERAL] = 390 * GI
    # few: a cpu request that only the emptiest nodes still hold — the largest free-cpu value that at most `most`
    # nodes reach (other filters can only lower the count; the case asserts what came out)
    valid = (cl.nodes["flags"] & abi.NODE_VALID) != 0
    free = [np.where(valid, cl.nodes["allocatable"][:, r] - st["requested"][:, r], 0) for r in (abi.RES_CPU, abi.RES_MEMORY)]

    def threshold(v, most):  # the smallest value of v that at most `most` entries reach (else the largest value)
        vals, counts = np.unique(v, return_counts=True)
        ok = np.nonzero(np.cumsum(counts[::-1])[::-1] <= most)[0]
        return max(int(vals[ok[0]] if len(ok) else vals[-1]), 1)

    few = synth.make_pods(2, seed=seed + 2)
    for j, most in enumerate((kc // 2, 3)):
        cpu = threshold(free[0], most)
        mem = threshold(np.where(free[0] >= cpu, free[1], 0), most)  # many equally empty nodes: memory narrows them
        few["requests"][j, abi.RES_CPU] = few["limits"][j, abi.RES_CPU] = cpu
        few["requests"][j, abi.RES_MEMORY] = few["limits"][j, abi.RES_MEMORY] = mem
        few["nonzero_requests"][j] = (cpu, mem)
    nowhere = few[:1].copy()
    nowhere["requests"][0, abi.RES_CPU] = nowhere["limits"][0, abi.RES_CPU] = 10_000_000
    nowhere["nonzero_requests"][0, 0] = 10_000_000
    return np.concatenate([mix, aux, few, nowhere]), len(mix) + len(aux), len(mix) + len(aux) + len(few)


def _run_records(cfg, batch, cl, warm, n_mix, seed, want_comb, want_lanes, table):
    """Loads cl, schedules `warm` on the device and in the oracle, then reads one queue's rounds back and checks every
    list and record against the oracle's keys on the same state.  → the geometry."""
    on, _, st = oracle.schedule_cluster(cfg, cl, warm, n_threads=16)
    with Engine(cfg, cl.n) as e:
        synth.load_into(e, cl)
        if len(warm):
            gn, _, _ = e.schedule(warm)
            np.testing.assert_array_equal(gn, on)
        e.stage(synth.make_pods(1, seed=1))
        kc = e.debug_round_records(0, 1)[0]["kc"]
        pods, i_few, i_nowhere = _probe_pods(cfg, cl, st, kc, n_mix, seed)
        e.stage(pods)
        before = e.read_state()
        out = []
        for first in range(0, len(pods), batch):
            nb = min(batch, len(pods) - first)
            geom, lists, recs = e.debug_round_records(first, nb)
            out.append((first, lists, recs))
        after = e.read_state()
        for k in before:
            np.testing.assert_array_equal(before[k], after[k], err_msg=f"{k}: the hook changed the table")
        with pytest.raises(KoordGPUError) as err:
            e.debug_round_records(len(pods) - 1, 2)
        assert err.value.code == abi.E_INVALID
    print(f"geometry at {cl.n} nodes ({table}): {geom}")  # the instantiation that ran, as the device reports it
    assert (geom["combined"], _wave_bucket(geom["n_lists"])) == (want_comb, want_lanes), geom
    _check_rounds(cfg, cl, st, pods, geom, out, i_few, i_nowhere, table)
    return geom


def _check_rounds(cfg, cl, st, pods, geom, out, i_few, i_nowhere, table):
    """Every list and record of `out` ([(first pod, lists, records)]) against the oracle's keys on state `st`; then the
    claims of the case."""
    kc = geom["kc"]
    n_feas, n_top, full, few_all = [], [], False, []
    for first, lists, recs in out:
        for j in range(len(recs)):
            what = f"{cl.n} nodes, {table}, pod {first + j}"
            kv = oracle.node_keys(cfg, cl.nodes, cl.metrics, st, pods[first + j], cl.now_ns, 0, cl.n)
            C.check_lists(lists[j], kv, geom, what)          # the wide pass alone
            mlists, model = M.round_record(kv, geom)
            C.check_record_exact(recs[j], model, kc, what, union=set(mlists.ravel().tolist()))  # the merge on them
            C.check_record(recs[j], kv, kc, what)             # and the record against the oracle alone
            feas = kv[kv != 0]
            n_feas.append(len(feas))
            n_top.append(int((feas >> np.uint64(32) == feas.max() >> np.uint64(32)).sum()) if len(feas) else 0)
            full |= bool((mlists != 0).all(axis=1).any())
            if not (mlists != 0).all(axis=1).any():  # no list full: nothing is left out of the lists
                assert int(recs[j][kc]) == (0 if len(feas) <= kc else int(np.sort(feas)[-kc - 1]) + 1), what
                assert np.count_nonzero(recs[j][:kc]) == min(len(feas), kc), what
                if 1 <= len(feas) < kc:
                    few_all.append(first + j)
    # the case is the case it claims to be (from the oracle's keys alone)
    assert n_feas[i_nowhere] == 0
    if cl.n > kc:
        assert any(1 <= f <= kc - 1 for f in n_feas[i_few:i_nowhere]), n_feas[i_few:i_nowhere]
    if cl.n > 8 * kc:  # (smaller clusters need not have kc feasible nodes at all)
        # a pod with 1 .. kc - 1 feasible nodes and no full list: its record lists them all and ub == 0 (above)
        assert any(i_few <= j < i_nowhere for j in few_all), (few_all, n_feas[i_few:i_nowhere])
        if table == "ties":
            assert max(n_top) > kc
        else:
            assert max(n_feas) > kc and full


@pytest.mark.parametrize("n,comb,lanes,table,shape,weights", _real_cases())
def test_round_records_real_tables(n, comb, lanes, table, shape, weights):
    cfg = _cfg(*weights, batch=shape[0], ppw=shape[1])
    cl = _cluster(n, table, seed=n + 12)
    big = n > 40_000
    warm = synth.make_pods(min(300 if table != "ties" else 150, 2 * n), seed=n + 13)
    geom = _run_records(cfg, shape[0], cl, warm, 8 if big or shape[0] == 1 else 28, n + 14, comb, lanes, table)
    assert geom["score_bits"] == {(1, 1): 8, (3, 11): 11, (41, 41): 14, (40, 41): 13}[weights]


@pytest.mark.parametrize("plugin", [framework.NODE_NUMA_RESOURCE, framework.DEVICE_SHARE, framework.RESERVATION])
def test_round_records_refuses_other_profiles(plugin):
    """The hook reads the Fit + LoadAware round engine only: the NUMA, DeviceShare and exact-pass profiles write other
    lists, which the model does not describe."""
    prof = framework.Profile(filter=(FIT, LA, plugin), score={FIT: 1, LA: 1, plugin: 1})
    with Engine(framework.build_config(profile=prof), 64) as e:
        with pytest.raises(KoordGPUError) as err:
            e.debug_round_records(0, 1)
        assert err.value.code == abi.E_UNSUPPORTED


def test_round_records_largest_table():
    """524,288 nodes, the engine's largest table: 512 group lists, 8 per lane.  One case, 16 pods."""
    n = 524_288
    cfg = _cfg(1, 1, batch=16, ppw=8)
    cl = _cluster(n, "random", seed=99)
    _run_records(cfg, 16, cl, synth.make_pods(0, seed=1), 9, 98, 1, 8, "random")
