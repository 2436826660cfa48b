"""One pod record (LonePod), three views: kg_pods_evaluate_reservation, kg_pods_diagnose and kg_debug_topn run the same
per-node body over the same decoded pod, so on the subset where the first evaluates what the other two evaluate — the
shipped profile (no default plugins) and pods without ephemeral-storage / scalar requests — their feasible sets are
one set.  And the entry points' scratch buffers, laid out per call and grown on demand, survive regrowth and
interleaving: each call on a long-lived engine equals the same call made first on a fresh engine, and the scheduling
pass afterwards equals the oracle."""
import functools

import numpy as np
import pytest

import test_shipped_profile as SP
from koordinator_amd import Engine, abi, synth

pytestmark = pytest.mark.gpu

N_NODES = 257  # two node blocks, the second with one node


@functools.lru_cache(maxsize=None)
def _table():
    """257 nodes of the shipped profile's cluster and a queue without quotas; built once, left unchanged"""
    cfg = SP.config()
    cluster, numa, dev, rsv, pods, _ = SP.workload(N_NODES, 160, 8101)
    pods["quota_id"] = 0
    assert not pods["requests"][:, abi.RES_EPHEMERAL:].any()  # no aux requests: evaluate_reservation skips them
    return cfg, cluster, numa, dev, rsv, pods


def _engine():
    cfg, cluster, numa, dev, rsv, _ = _table()
    e = Engine(cfg, cluster.n)
    synth.load_shipped_into(e, cluster, numa, dev, rsv, None)
    return e


def _eight():
    """8 pods of the queue: two that require a reservation, two with GPU requests, two cpuset pods, two plain"""
    pods = _table()[5]
    need = np.flatnonzero(pods["reservation_flags"] & abi.POD_RSV_AFFINITY)
    gpu = np.flatnonzero(pods["device_requests"].any(axis=1))
    cpuset = np.flatnonzero((pods["qos"] == abi.QOS["LSR"]) & ~pods["device_requests"].any(axis=1))
    plain = np.flatnonzero((pods["qos"] != abi.QOS["LSR"]) & ~pods["device_requests"].any(axis=1) &
                           (pods["reservation_flags"] == 0))
    sel = []
    for group in (need, gpu, cpuset, plain):
        sel += [int(k) for k in group if int(k) not in sel][:2]
    assert len(sel) == 8
    return pods[sel]


def test_three_views_of_one_pod_agree():
    pods = _eight()
    with _engine() as e:
        diag, status = e.diagnose(pods, node_status=True)
        some = 0
        for k in range(len(pods)):
            ev = e.evaluate_reservation(pods[k])
            rows, feasible = e.debug_topn(pods[k], 64)
            ok = ev["pass"] != 0
            assert np.array_equal(ok, status[k] == 0), k
            assert int(ok.sum()) == int(diag["feasible"][k]) == feasible, k
            assert len(rows) == min(64, feasible)
            assert ok[rows["node_idx"]].all() and (status[k][rows["node_idx"]] == 0).all(), k
            some += 0 < feasible < N_NODES
    assert some >= 4  # the feasible sets are neither empty nor everything for most of the pods


def _preempt_args(n_cand, empty=None):
    """candidates 0..n_cand-1 with the nodes' own pods as potential victims (candidate `empty` has none)"""
    cluster = _table()[1]
    nodes = np.arange(n_cand, dtype=np.int32)
    vics = [cluster.existing_pods[cluster.existing_node == i] for i in nodes]
    if empty is not None:
        vics[empty] = vics[empty][:0]
    prios = [(np.arange(len(v)) % 3).astype(np.int32) * 100 for v in vics]
    starts = [np.full(len(v), 17 * 10**17, dtype=np.int64) + np.arange(len(v)) for v in vics]
    return nodes, vics, prios, starts


def _calls():
    """(name, call(engine) -> bytes of everything the call returns), in the order they run on the long-lived engine"""
    pods = _table()[5]
    eight = _eight()
    big = eight[3:4].copy()  # a GPU pod as the preemptor, with more cpu than most nodes have free
    big["requests"][0, abi.RES_CPU] = big["nonzero_requests"][0, 0] = 64000
    big["reservation_flags"] = 0

    def flat(x):
        if isinstance(x, dict):
            return b"".join(flat(x[k]) for k in sorted(x))
        if isinstance(x, (tuple, list)):
            return b"".join(flat(v) for v in x)
        return np.ascontiguousarray(x).tobytes()

    return [
        ("diagnose 1", lambda e: flat(e.diagnose(pods[:1]))),
        ("diagnose 65 + status", lambda e: flat(e.diagnose(pods[:65], node_status=True))),
        ("topn 1", lambda e: flat(e.debug_topn(eight[0], 1))),
        ("topn 64", lambda e: flat(e.debug_topn(eight[4], 64))),
        ("evaluate_reservation", lambda e: flat(e.evaluate_reservation(eight[1]))),
        ("preempt 1", lambda e: flat(e.preempt(big, *_preempt_args(1), want_reject=True))),
        ("preempt 65, one empty", lambda e: flat(e.preempt(big, *_preempt_args(65, empty=7), want_reject=True))),
        ("diagnose 1 again", lambda e: flat(e.diagnose(pods[:1]))),
    ]


def test_buffers_survive_regrowth_and_interleaving():
    cfg, cluster, numa, dev, rsv, pods = _table()
    calls = _calls()
    want = []
    for _, call in calls:  # each call as the first call of a fresh engine
        with _engine() as e:
            want.append(call(e))
    assert want[0] == want[-1]
    queue = pods[100:124]
    w = SP.oracle_run(cfg, cluster, numa, dev, rsv, queue, None)
    with _engine() as e:
        for (name, call), expected in zip(calls, want):
            assert call(e) == expected, name
        node, score, _ = e.schedule(queue)
        slot, minors = e.fetch_reservations(0, len(queue)), e.fetch_devices(0, len(queue))
    assert np.array_equal(node, w["node"]) and np.array_equal(score, w["score"])
    assert np.array_equal(slot, w["slot"]) and np.array_equal(minors, w["minors"])
    assert (node >= 0).any()
