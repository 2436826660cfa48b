"""kg_pods_diagnose on the device: framework.FitError of many pods per call (NumAllNodes, the NodeToStatusMap reasons
histogram, the nodes per first-failing plugin), against the oracle.

The expected per-node word is what RunFilterPlugins leaves in the NodeToStatusMap: the first failing plugin in the
profile's Filter order (TaintToleration, NodeAffinity, NodeResourcesFit, LoadAwareScheduling, NodeNUMAResource,
DeviceShare, Reservation) with all of its reasons and none of the later plugins'.  It is composed from the oracle's
existing per-plugin functions only.  Every check compares the per-node words first (node_status=True), then
reason_nodes / plugin_nodes / feasible / num_all_nodes against counts of that same expected matrix, then the invariants
the header states.

Wide profile: oracle.fit_filter bits, else REJECT_LOADAWARE from oracle.loadaware_filter; feasible also equals the
count of non-zero oracle.node_keys.  Default-plugin profile: oracle.default_plugins' taint_filter / affinity_filter in
front of Fit.  Shipped profile: oracle.rsv_restore per node, Fit / LoadAware on the restored state, oracle.numa_eval on
the restored Requested, oracle.ds_filter.  The oracle has no per-node function for the Reservation Filter of a pod that
requires a reservation, so that one bit comes from Engine.evaluate_reservation (as test_debug_topn.py takes the
nomination from it): on nodes every earlier plugin passes, KG_REJECT_RESERVATION is checked device against device.
Whether such a pod has no feasible node at all is pinned through the oracle's own loop (SP.oracle_run of the pod alone).

No side effects: a queue scheduled with diagnose calls in the middle equals the uninterrupted oracle run."""
import dataclasses
import functools

import numpy as np
import pytest

import test_debug_topn as TD
import test_shipped_profile as SP
from koordinator_amd import Engine, abi, framework as F, synth
from koordinator_amd.abi import KoordGPUError
from koordinator_amd.engine import Loopback
from oracle import oracle

pytestmark = pytest.mark.gpu

DIAG_CHUNK = 64  # kDiagChunk (csrc/diag_dev.h): the pods of one diag_eval launch
GI = 1 << 30
WIDE_N = (1, 5, 63, 65, 257, 1500)
FIT_BITS = abi.REJECT_FIT_PODS | abi.REJECT_FIT_CPU | abi.REJECT_FIT_MEMORY | abi.REJECT_FIT_OTHER
# single-bit plugins: column -> bit
ONE_BIT = {abi.PL_LOADAWARE: abi.REJECT_LOADAWARE, abi.PL_NUMA: abi.REJECT_NUMA, abi.PL_DEVICESHARE: abi.REJECT_DEVICE,
           abi.PL_RESERVATION: abi.REJECT_RESERVATION, abi.PL_TAINT: abi.REJECT_TAINT,
           abi.PL_NODE_AFFINITY: abi.REJECT_NODE_AFFINITY}
# framework order: the first plugin whose bits are set gives the status
ORDER = (abi.REJECT_TAINT, abi.REJECT_NODE_AFFINITY, FIT_BITS, abi.REJECT_LOADAWARE, abi.REJECT_NUMA, abi.REJECT_DEVICE,
         abi.REJECT_RESERVATION)


def first_failure(fails: int) -> int:
    """The status word of a node from the bits of every plugin that fails on it."""
    for mask in ORDER:
        if fails & mask:
            return fails & mask
    return 0


def expected_diag(words: np.ndarray) -> np.ndarray:
    """FIT_DIAG_DTYPE records counted from the expected (pods, nodes) status words."""
    out = np.zeros(len(words), dtype=abi.FIT_DIAG_DTYPE)
    valid = words != abi.REJECT_INVALID_NODE
    out["num_all_nodes"] = valid.sum(axis=1)
    out["feasible"] = (words == 0).sum(axis=1)
    for b in range(abi.DIAG_REASONS):
        out["reason_nodes"][:, b] = (valid & ((words >> b) & 1 != 0)).sum(axis=1)
    out["plugin_nodes"][:, abi.PL_FIT] = (valid & ((words & FIT_BITS) != 0)).sum(axis=1)
    for col, bit in ONE_BIT.items():
        out["plugin_nodes"][:, col] = (valid & ((words & bit) != 0)).sum(axis=1)
    return out


def check_invariants(diag, possible_bits: int):
    for d in diag:
        assert d["feasible"] + d["plugin_nodes"].sum() == d["num_all_nodes"]
        for col, bit in ONE_BIT.items():
            assert d["plugin_nodes"][col] == d["reason_nodes"][bit.bit_length() - 1]
        fit = [int(d["reason_nodes"][b]) for b in (0, 1, 2, 7)]
        assert max(fit) <= d["plugin_nodes"][abi.PL_FIT] <= sum(fit)
        for b in range(abi.DIAG_REASONS):
            if not (possible_bits >> b) & 1:
                assert d["reason_nodes"][b] == 0, b
        assert not d["plugin_nodes"][abi.PL_BALANCED:].any()


def check_against(diag, status, words, possible_bits):
    """Per-node words first, then every count against the same expected matrix, then the invariants."""
    assert status.shape == words.shape and status.dtype == np.int32
    bad = np.argwhere(status != words)
    assert bad.size == 0, f"first differing (pod, node) {bad[0]}: device {status[tuple(bad[0])]} expected {words[tuple(bad[0])]}"
    want = expected_diag(words)
    for f in ("num_all_nodes", "feasible", "reason_nodes", "plugin_nodes"):
        assert np.array_equal(diag[f], want[f]), f
    check_invariants(diag, possible_bits)


# ---------------------------------------------------------------------------------------------------------------
# wide profile
# ---------------------------------------------------------------------------------------------------------------
WIDE_BITS = FIT_BITS | abi.REJECT_LOADAWARE


@functools.lru_cache(maxsize=None)
def _wide(n):
    """The n-node cluster (every 7th node full by pod count, 70 % of the nodes with ephemeral-storage, two deleted
    slots from 5 / 257 nodes on), the pods — three stock ones and seven sized from the cluster's free resources — the
    oracle state with the existing pods added, and per (pod, node) the Fit bits, the LoadAware verdict and the expected
    status word.  Computed once per n, shared and left unchanged."""
    cfg = F.build_config()
    base = synth.make_cluster(n, seed=5101 + n)
    st = oracle.states(n)
    oracle.add_pods(cfg, st, base.existing_pods, base.existing_node)
    nodes = base.nodes.copy()
    nodes["allowed_pods"][::7] = st["num_pods"][::7]  # Too many pods
    rng = np.random.default_rng(5300 + n)
    nodes["allocatable"][:, abi.RES_EPHEMERAL] = np.where(rng.random(n) < 0.7, 100 * GI, 0)
    dead = [k for k in (2, 64) if k < n - 1 and n >= 5]
    cluster = dataclasses.replace(base, nodes=nodes)
    onodes = nodes.copy()  # the oracle's view: the deleted slots are invalid
    onodes["flags"][dead] &= ~abi.NODE_VALID
    alloc, req = nodes["allocatable"], st["requested"]
    free_cpu = np.maximum(alloc[:, abi.RES_CPU] - req[:, abi.RES_CPU], 0)
    free_mem = np.maximum(alloc[:, abi.RES_MEMORY] - req[:, abi.RES_MEMORY], 0)
    cpu = max(int(np.median(free_cpu)), 1)
    mem = max(int(np.percentile(free_mem, 60)), 1)
    crafted = [F.make_pod({"cpu": f"{cpu}m", "memory": str(GI)}),
               F.make_pod({"cpu": "100m", "memory": str(mem)}),
               F.make_pod({"cpu": f"{cpu}m", "memory": str(mem)}),
               F.make_pod({"cpu": "1000", "memory": str(GI)}),  # nothing fits
               F.make_pod({}),
               F.make_pod({"cpu": "100m", "memory": str(GI), "ephemeral-storage": str(10 * GI)}),
               F.make_pod({"cpu": f"{cpu}m", "memory": str(mem), "ephemeral-storage": str(200 * GI)})]
    pods = np.concatenate([synth.make_pods(3, seed=5200 + n)] + crafted)
    fit = np.zeros((len(pods), n), dtype=np.int32)
    la = np.zeros((len(pods), n), dtype=bool)
    words = np.zeros((len(pods), n), dtype=np.int32)
    for j in range(len(pods)):
        pod = pods[j:j + 1]
        for i in range(n):
            nd = onodes[i:i + 1]
            if not nd["flags"][0] & abi.NODE_VALID:
                words[j, i] = abi.REJECT_INVALID_NODE
                continue
            fit[j, i] = oracle.fit_filter(nd, st[i:i + 1], pod)
            la[j, i] = oracle.loadaware_filter(cfg, nd, cluster.metrics[i:i + 1], pod, cluster.now_ns) != 0
            words[j, i] = first_failure(int(fit[j, i]) | (abi.REJECT_LOADAWARE if la[j, i] else 0))
    keys = np.stack([oracle.node_keys(cfg, onodes, cluster.metrics, st, pods[j], cluster.now_ns, 0, n) != 0
                     for j in range(len(pods))])
    return cfg, cluster, dead, pods, fit, la, words, keys


def _wide_batches(n):
    """(pod indices) of the three batches: 1, 2 and one larger than the internal chunk (the ten pods repeated)."""
    k = len(_wide(n)[3])
    return [0], [2, 1], [q % k for q in range(DIAG_CHUNK + 6)]


@functools.lru_cache(maxsize=None)
def _wide_engine(n):
    """One engine per n: every batch with and without node_status, and debug_topn's feasible count per pod."""
    cfg, cluster, dead, pods, *_ = _wide(n)
    with Engine(cfg, n) as e:
        synth.load_into(e, cluster)
        if dead:
            e.delete_nodes(dead)
        assert e.num_nodes == n
        got = [(e.diagnose(pods[b], node_status=True), e.diagnose(pods[b])) for b in _wide_batches(n)]
        topn = [e.debug_topn(pods[j], 1)[1] for j in range(len(pods))]
    return got, topn


def test_wide_inputs_cover_the_edges():
    """On the oracle side alone: the chosen inputs produce every bit the profile can produce, a node with two Fit
    reasons, a node failing both Fit and LoadAware (LoadAware must not be counted there), LoadAware as the first
    failure, an invalid slot, and a pod without a feasible node.  If this fails the inputs are wrong, not the engine."""
    seen = 0
    multi = both = la_first = invalid = nofit = some = False
    for n in WIDE_N:
        _, _, _, _, fit, la, words, _ = _wide(n)
        valid = words != abi.REJECT_INVALID_NODE
        seen |= int(np.bitwise_or.reduce(np.where(valid, words, 0), axis=None))
        multi |= bool(((fit & (fit - 1)) != 0).any())
        both |= bool(((fit != 0) & la).any())
        la_first |= bool((words == abi.REJECT_LOADAWARE).any())
        invalid |= bool((~valid).any())
        nofit |= bool(((words == 0).sum(axis=1) == 0).any())
        some |= bool(((words == 0).sum(axis=1) > 0).any())
    assert seen == WIDE_BITS
    assert multi and both and la_first and invalid and nofit and some


@pytest.mark.parametrize("n", WIDE_N)
def test_wide_profile_counts_equal_oracle(n):
    _, _, _, pods, _, _, words, keys = _wide(n)
    got, topn = _wide_engine(n)
    assert np.array_equal((words == 0).sum(axis=1), keys.sum(axis=1))  # the oracle's own feasible set
    for b, ((diag, status), plain) in zip(_wide_batches(n), got):
        check_against(diag, status, words[b], WIDE_BITS)
        assert plain.tobytes() == diag.tobytes()  # the counts do not depend on the status copy
    # agreement with the rest of the engine (a cross-check only): kg_debug_topn's feasible count
    diag = got[2][0][0]
    assert [int(v) for v in diag["feasible"][:len(pods)]] == topn


def test_wide_feasible_zero_iff_schedule_alone_fails():
    """feasible == 0 exactly when kg_pods_schedule of that pod alone, on a fresh copy of the cluster, returns -1."""
    n = 257
    cfg, cluster, dead, pods, *_ = _wide(n)
    diag = _wide_engine(n)[0][2][0][0]
    outcomes = set()
    for j in range(len(pods)):
        with Engine(cfg, n) as e:
            synth.load_into(e, cluster)
            e.delete_nodes(dead)
            node = int(e.schedule(pods[j:j + 1])[0][0])
        assert (diag["feasible"][j] == 0) == (node < 0), j
        outcomes.add(node < 0)
    assert outcomes == {True, False}


# ---------------------------------------------------------------------------------------------------------------
# upstream default plugins: TaintToleration / NodeAffinity in front of NodeResourcesFit
# ---------------------------------------------------------------------------------------------------------------
DEFAULTS_BITS = WIDE_BITS | abi.REJECT_TAINT | abi.REJECT_NODE_AFFINITY


@functools.lru_cache(maxsize=None)
def _defaults():
    cluster, pods, preds, picks = TD._defaults_world()
    cfg = F.build_config(profile=TD.DEFAULTS_PROFILE)
    st = oracle.states(cluster.n)
    oracle.add_pods(cfg, st, cluster.existing_pods, cluster.existing_node)
    hard = np.flatnonzero((pods["n_required_terms"] > 0) | (pods["node_selector"] != 0))
    sel = sorted(set(picks) | {int(j) for j in hard[:9]})
    big = pods[sel[:2]].copy()  # no node has 1000 free cores: NodeResourcesFit fails behind the two default plugins
    big["requests"][:, abi.RES_CPU] = big["nonzero_requests"][:, 0] = 1_000_000
    chosen = np.concatenate([pods[sel], big])
    fails = np.zeros((len(chosen), cluster.n), dtype=np.int32)
    for k in range(len(chosen)):
        pod = chosen[k:k + 1]
        for i in range(cluster.n):
            nd = cluster.nodes[i:i + 1]
            d = oracle.default_plugins(preds[i], pod)
            fails[k, i] = (0 if d["taint_filter"] else abi.REJECT_TAINT) | \
                (0 if d["affinity_filter"] else abi.REJECT_NODE_AFFINITY) | oracle.fit_filter(nd, st[i:i + 1], pod) | \
                (abi.REJECT_LOADAWARE if oracle.loadaware_filter(cfg, nd, cluster.metrics[i:i + 1], pod, cluster.now_ns)
                 else 0)
    words = np.vectorize(first_failure, otypes=[np.int32])(fails)
    return cfg, cluster, preds, chosen, fails, words


def test_default_plugins_profile_counts_equal_oracle():
    cfg, cluster, preds, pods, fails, words = _defaults()
    # oracle side: both default plugins occur as the first failure, and some node fails both (taint only is reported)
    assert (words == abi.REJECT_TAINT).any() and (words == abi.REJECT_NODE_AFFINITY).any()
    both = (fails & abi.REJECT_TAINT != 0) & (fails & abi.REJECT_NODE_AFFINITY != 0)
    assert both.any() and (words[both] == abi.REJECT_TAINT).all()
    assert ((fails & abi.REJECT_TAINT != 0) & (fails & FIT_BITS != 0)).any()
    with Engine(cfg, cluster.n) as e:
        synth.load_into(e, cluster)
        e.upsert_predicates(preds)
        diag, status = e.diagnose(pods, node_status=True)
        topn = [e.debug_topn(q, 1)[1] for q in pods]
    check_against(diag, status, words, DEFAULTS_BITS)
    assert [int(v) for v in diag["feasible"]] == topn


# ---------------------------------------------------------------------------------------------------------------
# shipped profile
# ---------------------------------------------------------------------------------------------------------------
SHIPPED_BITS = WIDE_BITS | abi.REJECT_NUMA | abi.REJECT_DEVICE | abi.REJECT_RESERVATION


def _shipped_fails(cfg, cluster, numa, dev, rsv, st, pod):
    """Per node the bits of every plugin before Reservation that fails, composed as test_debug_topn._shipped_parts does:
    oracle.rsv_restore, NodeResourcesFit / LoadAware on the restored NodeInfo, oracle.numa_eval on the restored
    Requested, oracle.ds_filter on the node's devices."""
    n = cluster.n
    fails = np.zeros(n, dtype=np.int32)
    alloc = cluster.nodes["allocatable"]
    for i in range(n):
        nd, mt = cluster.nodes[i:i + 1], cluster.metrics[i:i + 1]
        rs = oracle.rsv_restore(rsv[i], st[i:i + 1], pod)
        s = st[i:i + 1].copy()
        s["requested"][0, :2] = rs["requested_cpu"], rs["requested_mem"]
        s["nonzero"][0] = rs["nonzero_cpu"], rs["nonzero_mem"]
        s["num_pods"][0] = rs["num_pods"]
        f = oracle.fit_filter(nd, s, pod)
        if oracle.loadaware_filter(cfg, nd, mt, pod, cluster.now_ns) != 0:
            f |= abi.REJECT_LOADAWARE
        if not oracle.numa_eval(cfg, numa[i:i + 1], pod, (rs["requested_cpu"], rs["requested_mem"]), alloc[i, :2])[0]:
            f |= abi.REJECT_NUMA
        if not oracle.ds_filter(dev[i:i + 1], pod):
            f |= abi.REJECT_DEVICE
        fails[i] = f
    return fails


@functools.lru_cache(maxsize=None)
def _shipped():
    """The workload, the diagnosed pods — the 16 pods with a required reservation affinity, every 12th pod, and a GPU
    pod and a cpuset pod with cpu raised to the cluster's median free cpu (Fit ahead of NodeNUMAResource / DeviceShare
    on restored rows) — and their oracle-side plugin failures."""
    cfg = SP.config()
    cluster, numa, dev, rsv, pods, _ = SP.workload(600, 300, 4321)
    pods["quota_id"] = 0
    st = oracle.states(cluster.n)
    oracle.add_pods(cfg, st, cluster.existing_pods, cluster.existing_node)
    need = np.flatnonzero(pods["reservation_flags"] & abi.POD_RSV_AFFINITY)
    sel = sorted(set(int(j) for j in need) | set(range(0, len(pods), 12)))
    free_cpu = cluster.nodes["allocatable"][:, abi.RES_CPU] - st["requested"][:, abi.RES_CPU]
    cpu = max(int(np.median(free_cpu)) // 1000, 1) * 1000  # whole cores: a cpuset pod stays a valid cpuset pod
    gpu = int(np.flatnonzero(pods["device_requests"].any(axis=1))[0])
    cpuset = int(np.flatnonzero((pods["qos"] == abi.QOS["LSR"]) & ~pods["device_requests"].any(axis=1))[0])
    big = pods[[gpu, cpuset]].copy()
    big["requests"][:, abi.RES_CPU] = cpu
    big["nonzero_requests"][:, 0] = cpu
    big["reservation_flags"] = 0
    chosen = np.concatenate([pods[sel], big])
    fails = np.stack([_shipped_fails(cfg, cluster, numa, dev, rsv, st, chosen[k:k + 1]) for k in range(len(chosen))])
    return cfg, cluster, numa, dev, rsv, chosen, fails


def test_shipped_inputs_cover_the_edges():
    """Oracle side alone: NodeNUMAResource and DeviceShare each occur as the first failure, some node fails both (it
    must count as NodeNUMAResource only), and NodeResourcesFit fails ahead of either on restored rows."""
    *_, fails = _shipped()
    numa, ds, fit = fails & abi.REJECT_NUMA != 0, fails & abi.REJECT_DEVICE != 0, fails & FIT_BITS != 0
    early = fails & (FIT_BITS | abi.REJECT_LOADAWARE) != 0
    assert (numa & ~early).any() and (ds & ~numa & ~early).any() and (numa & ds & ~early).any()
    assert (fit & numa).any() and (fit & ds).any()


def test_shipped_profile_counts_equal_oracle_composition():
    """The Reservation bit of a pod that requires a reservation is taken from Engine.evaluate_reservation on the nodes
    every earlier plugin passes: that one bit is device against device.  Its `pass` word is used, which for a pod
    without device requests equals "no slot nominated" (asserted); for a pod with device requests the nominated word is
    also -1 where the Reservation Filter passed and DeviceShare's FilterReservation then dropped every satisfied slot,
    which is no Filter failure.  feasible == 0 for such a pod must match the oracle's own loop (SP.oracle_run of the
    pod alone returning -1)."""
    cfg, cluster, numa, dev, rsv, pods, fails = _shipped()
    need = (pods["reservation_flags"] & abi.POD_RSV_AFFINITY) != 0
    assert need.sum() == 16
    with Engine(cfg, cluster.n) as e:
        synth.load_shipped_into(e, cluster, numa, dev, rsv, None)
        diag, status = e.diagnose(pods, node_status=True)
        plain = e.diagnose(pods)
        ev = {int(k): e.evaluate_reservation(pods[k]) for k in np.flatnonzero(need)}
        topn = [e.debug_topn(q, 1)[1] for q in pods]
    all_fails = fails.copy()
    for k, v in ev.items():
        rejected = (fails[k] == 0) & (v["pass"] == 0)
        if not pods["device_requests"][k].any():  # the nominated word says the same: no satisfied slot, none nominated
            assert np.array_equal(rejected, (fails[k] == 0) & (v["nominated"] < 0))
        all_fails[k] |= np.where(rejected, abi.REJECT_RESERVATION, 0).astype(np.int32)
    words = np.vectorize(first_failure, otypes=[np.int32])(all_fails)
    check_against(diag, status, words, SHIPPED_BITS)
    assert plain.tobytes() == diag.tobytes()
    assert (diag["reason_nodes"][:, 8] > 0).any()  # the Reservation Filter does reject here
    assert [int(v) for v in diag["feasible"]] == topn
    for k in np.flatnonzero(need):
        w = SP.oracle_run(cfg, cluster, numa, dev, rsv, pods[k:k + 1], None, n_threads=1)
        assert (diag["feasible"][k] == 0) == (w["node"][0] < 0), k


def test_shipped_feasible_zero_iff_schedule_alone_fails():
    cfg, cluster, numa, dev, rsv, pods, _ = _shipped()
    with Engine(cfg, cluster.n) as e:
        synth.load_shipped_into(e, cluster, numa, dev, rsv, None)
        feasible = e.diagnose(pods)["feasible"]
    zero, some = np.flatnonzero(feasible == 0), np.flatnonzero(feasible > 0)
    for k in list(zero[:2]) + list(some[:2]):
        with Engine(cfg, cluster.n) as e:
            synth.load_shipped_into(e, cluster, numa, dev, rsv, None)
            node = int(e.schedule(pods[k:k + 1])[0][0])
        assert (feasible[k] == 0) == (node < 0), k


# ---------------------------------------------------------------------------------------------------------------
# no side effects
# ---------------------------------------------------------------------------------------------------------------
def test_wide_schedule_unchanged_by_diagnose_calls():
    cfg = F.build_config(pipeline_depth=3)
    cluster = synth.make_cluster(3000, seed=5401)
    pods = synth.make_pods(400, seed=5402)
    want, want_score, st = oracle.schedule_cluster(cfg, cluster, pods, 8)
    with Engine(cfg, cluster.n) as e:
        synth.load_into(e, cluster)
        e.stage(pods)
        e.schedule_staged(0, 200)
        first = e.diagnose(pods[200:280])
        e.diagnose(np.concatenate([pods[:7], synth.make_pods(3, seed=5403)]), node_status=True)
        again = e.diagnose(pods[200:280])
        e.schedule_staged(200, 200)
        node, score = e.fetch(0, len(pods))
        state = e.read_state()
    assert first.tobytes() == again.tobytes()
    assert np.array_equal(node, want) and np.array_equal(score, want_score)
    assert (first["feasible"][0] > 0) == (want[200] >= 0)  # pod 200 was the next pod when it was diagnosed
    assert np.array_equal(state["requested_cpu"], st["requested"][:, abi.RES_CPU])
    assert np.array_equal(state["requested_mem"], st["requested"][:, abi.RES_MEMORY])
    assert np.array_equal(state["la_est_cpu"], st["la_est_all"][:, 0])


def test_shipped_schedule_unchanged_by_diagnose_calls():
    cfg = SP.config()
    cluster, numa, dev, rsv, pods, quotas = SP.workload(500, 400, 5411)
    w = SP.oracle_run(cfg, cluster, numa, dev, rsv, pods, quotas)
    k = 200
    with Engine(cfg, cluster.n) as e:
        synth.load_shipped_into(e, cluster, numa, dev, rsv, quotas)
        e.stage(pods)
        e.schedule_staged(0, k)
        first = e.diagnose(pods[k:k + 70])
        e.diagnose(np.concatenate([pods[:5], SP.workload(500, 3, 5412)[4]]), node_status=True)
        again = e.diagnose(pods[k:k + 70])
        e.schedule_staged(k, len(pods) - k)
        node, score = e.fetch(0, len(pods))
        slot, minors, cpus = e.fetch_reservations(0, len(pods)), e.fetch_devices(0, len(pods)), e.fetch_cpusets(0, len(pods))
        state, used, rs = e.read_state(), e.read_devices(), e.read_reservations()
        ga, gc, gm = e.read_numa()
    assert first.tobytes() == again.tobytes()
    assert np.array_equal(node, w["node"]) and np.array_equal(score, w["score"])
    assert np.array_equal(slot, w["slot"]) and np.array_equal(minors, w["minors"]) and np.array_equal(cpus, w["cpus"])
    assert np.array_equal(state["requested_cpu"], w["st"]["requested"][:, abi.RES_CPU])
    assert np.array_equal(state["requested_mem"], w["st"]["requested"][:, abi.RES_MEMORY])
    assert np.array_equal(used[2], w["dev"]["used_ratio"])
    assert np.array_equal(rs[0], w["rsv"]["allocated_cpu"]) and np.array_equal(rs[2], w["rsv"]["assigned"])
    wa, wc, wm = oracle.numa_state_read(w["numa"], cluster.n)
    assert np.array_equal(ga, wa) and np.array_equal(gc, wc) and np.array_equal(gm, wm)


# ---------------------------------------------------------------------------------------------------------------
# refusals and edges
# ---------------------------------------------------------------------------------------------------------------
def test_scheduler_fit_error_message():
    """Scheduler.fit_error: the device counts rendered as FitError.Error() does."""
    n = 257
    cfg, cluster, dead, pods, _, _, words, _ = _wide(n)
    j = 6  # cpu 1000: nothing fits
    s = F.Scheduler(cfg, n)
    try:
        synth.load_into(s.engine, cluster)
        s.engine.delete_nodes(dead)
        assert s.schedule_pod(pods[j]).suggested_host == -1
        err = s.fit_error(pods[j])
    finally:
        s.close()
    want = expected_diag(words[j:j + 1])[0]
    assert err.num_all_nodes == n - len(dead) and err.feasible_nodes == 0
    assert err.unschedulable_plugins == {F.NODE_RESOURCES_FIT}
    assert err.reasons["Insufficient cpu"] == int(want["reason_nodes"][1]) == n - len(dead)
    assert err.reasons["Too many pods"] == int(want["reason_nodes"][0]) > 0
    assert err.message().startswith(f"0/{n - len(dead)} nodes are available: ")
    assert f"{n - len(dead)} Insufficient cpu" in err.message() and err.message().endswith(".")


def test_edges_and_refusals():
    cluster = synth.make_cluster(50, seed=5501)
    pods = synth.make_pods(6, seed=5502)
    cfg = F.build_config()
    with Engine(cfg, cluster.n) as e:
        # an empty table: every pod gets an all-zero record
        diag, status = e.diagnose(pods, node_status=True)
        assert len(diag) == 6 and not diag.view(np.int64).any() and status.shape == (6, 0)
        synth.load_into(e, cluster)
        # n == 0
        diag, status = e.diagnose(pods[:0], node_status=True)
        assert len(diag) == 0 and status.shape == (0, cluster.n)
        assert e.lib.kg_pods_diagnose(e.h, None, 0, None, None) == 0
        # null arguments
        out = np.zeros(6, dtype=abi.FIT_DIAG_DTYPE)
        one = np.ascontiguousarray(pods[:1])
        assert e.lib.kg_pods_diagnose(None, one.ctypes.data, 1, out.ctypes.data, None) == abi.E_INVALID
        assert e.lib.kg_pods_diagnose(e.h, None, 1, out.ctypes.data, None) == abi.E_INVALID
        assert e.lib.kg_pods_diagnose(e.h, one.ctypes.data, 1, None, None) == abi.E_INVALID
        assert e.lib.kg_pods_diagnose(e.h, one.ctypes.data, -1, out.ctypes.data, None) == abi.E_INVALID
        # a bad pod at batch index 3, named in the message
        bad = pods.copy()
        bad["requests"][3, abi.RES_CPU] = -5
        with pytest.raises(KoordGPUError) as ei:
            e.diagnose(bad)
        assert ei.value.code == abi.E_INVALID and "pod 3" in str(ei.value)
        # a device-requesting pod without DeviceShare in the profile
        gpu = pods.copy()
        gpu["device_requests"][1, 0] = 100
        with pytest.raises(KoordGPUError) as ei:
            e.diagnose(gpu)
        assert ei.value.code == abi.E_UNSUPPORTED and "pod 1" in str(ei.value) and "DeviceShare" in str(ei.value)
        # the engine still answers
        assert e.diagnose(pods)["num_all_nodes"].tolist() == [cluster.n] * 6
    prof = F.Profile(filter=(F.NODE_RESOURCES_FIT, F.LOAD_AWARE, F.POD_TOPOLOGY_SPREAD),
                     score={F.NODE_RESOURCES_FIT: 1, F.LOAD_AWARE: 1, F.POD_TOPOLOGY_SPREAD: 2})
    with Engine(F.build_config(profile=prof), cluster.n) as e:
        synth.load_into(e, cluster)
        with pytest.raises(KoordGPUError) as ei:
            e.diagnose(pods)
        assert ei.value.code == abi.E_UNSUPPORTED and "PodTopologySpread" in str(ei.value)
    with Loopback(2) as lb:  # a 2-rank engine that shards nodes
        engines = [Engine(F.build_config(multi_rank="shard"), cluster.n, rank=r, n_ranks=2, loopback=lb) for r in range(2)]
        try:
            for e in engines:
                synth.load_into(e, cluster)
            with pytest.raises(KoordGPUError) as ei:
                engines[0].diagnose(pods)
            assert ei.value.code == abi.E_UNSUPPORTED and "ranks" in str(ei.value)
        finally:
            for e in engines:
                e.close()
