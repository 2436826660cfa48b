"""Plain model of NodeResourcesFit's RequestedToCapacityRatio scoring (kg_fit_shape_set) on top of the
committed oracle — TEST INFRASTRUCTURE.  The oracle scores Fit by LeastAllocated only and stays as it is; the rule is
upstream v1.24's requestedToCapacityRatioScorer over BuildBrokenLinearFunction, restated as published:

  shape: n >= 1 points (utilization, score), utilization strictly increasing in [0, 100], score in [0, 10], used x 10;
  raw(p): the first i with p <= U[i]; i == 0 -> S[0]; else S[i-1] + (S[i]-S[i-1]) * (p-U[i-1]) / (U[i]-U[i-1]) with Go's
          int64 division (truncating toward zero: the numerator is negative on a falling segment); past the last
          point S[n-1].  p is an integer: raw is a table lut[0..100]; p < 0 reads lut[0];
  each resource (cpu, memory) takes part when its weight and the node's allocatable are non-zero:
          u = 100 if req > cap else req * 100 // cap, req = NonZeroRequested_node + NonZeroRequest_pod; r = lut[u];
  s = sum(r * w), ws = sum(w) over the taking-part resources WITH r > 0; score = 0 when ws == 0, else
          int64(math.Round(float64(s) / float64(ws))) — round half away from zero.

`fit_score` is that in Python integers and one float division, one row at a time: the definition.  `fit_scores` is the
integer form (2s + ws) // (2ws) over all nodes in int64; tests/test_fit_shape_rule.py holds the two equal.

The scheduling helpers follow tests/fit_strategy_reference.py step for step (its make_key / nonzero_request /
initial_states / Result and the oracle calls are imported, the file itself is unchanged); only the Fit term differs, so
they take the keys function's `shape` where that file takes a strategy name.  `skip_rule_answer` is NOT the model: it is
what a resolver keeping the monotone rule of DESIGN.md §3.3 would answer (see that file)."""
from __future__ import annotations

import math

import numpy as np

import fit_strategy_reference as S
from fit_strategy_reference import KC, BANK, PROBE, Result, initial_states, key_node, make_key, nonzero_request  # noqa: F401
from koordinator_amd import abi
from oracle import oracle

RISING = [(0, 0), (100, 10)]            # the identity shape: bin-packing
FALLING = [(0, 10), (100, 0)]           # spreading
PEAKED = [(0, 0), (60, 10), (100, 0)]   # favour 60 % utilization


def go_div(a: int, b: int) -> int:
    """Go's int64 division: truncates toward zero (Python's // floors)"""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


def raw(shape, p: int) -> int:
    """BuildBrokenLinearFunction over shape's points with score x 10"""
    pts = [(int(u), int(s) * 10) for u, s in shape]
    for i, (u, s) in enumerate(pts):
        if p <= u:
            if i == 0:
                return pts[0][1]
            u0, s0 = pts[i - 1]
            return s0 + go_div((s - s0) * (p - u0), u - u0)
    return pts[-1][1]


def table(shape) -> list:
    return [raw(shape, p) for p in range(101)]


def utilization(req: int, cap: int) -> int:
    return 100 if req > cap else req * 100 // cap


def round_half_away(x: float) -> int:
    """Go's math.Round"""
    return int(math.floor(x + 0.5)) if x >= 0 else -int(math.floor(-x + 0.5))


def mean(s: int, ws: int) -> int:
    return 0 if ws == 0 else round_half_away(float(s) / float(ws))


def fit_score(shape, weights, alloc, nz_node, nz_pod) -> int:
    """NodeResourcesFit Score of one row; weights / alloc / nz_node / nz_pod: (cpu, memory)"""
    lut = table(shape)
    s = ws = 0
    for r in range(2):
        w, cap = int(weights[r]), int(alloc[r])
        if w == 0 or cap == 0:
            continue
        u = utilization(int(nz_node[r]) + int(nz_pod[r]), cap)
        v = lut[max(u, 0)]
        if v > 0:
            s += v * w
            ws += w
    return mean(s, ws)


def fit_scores(shape, weights, alloc, nz_node, nz_pod) -> np.ndarray:
    """fit_score over every node in int64, the rounded mean as (2s + ws) // (2ws): alloc, nz_node int64[n, 2] → int64[n]"""
    lut = np.array(table(shape), dtype=np.int64)
    alloc = np.asarray(alloc, dtype=np.int64)
    req = np.asarray(nz_node, dtype=np.int64) + np.asarray(nz_pod, dtype=np.int64)[None, :]
    assert (alloc >= 0).all() and (req >= 0).all() and int(alloc.max(initial=0)) < 1 << 55 and int(req.max(initial=0)) < 1 << 55
    s = np.zeros(len(alloc), dtype=np.int64)
    ws = np.zeros(len(alloc), dtype=np.int64)
    for r in range(2):
        w = int(weights[r])
        cap = alloc[:, r]
        safe = np.where(cap != 0, cap, 1)
        u = np.where(req[:, r] > cap, 100, np.minimum(req[:, r], cap) * 100 // safe)
        v = lut[np.clip(u, 0, 100)]
        part = (cap != 0) & (v > 0) if w else np.zeros(len(alloc), dtype=bool)
        s += np.where(part, v * w, 0)
        ws += np.where(part, w, 0)
    return np.where(ws != 0, (2 * s + ws) // np.where(ws != 0, 2 * ws, 1), 0)


def keys(cfg, cluster, st, pod, shape, lo: int = 0, hi: int | None = None) -> np.ndarray:
    """packed keys of `pod` on nodes [lo, hi) of the current state under RequestedToCapacityRatio with `shape`"""
    hi = cluster.n if hi is None else hi
    kv = oracle.node_keys(S._cfg_no_fit_score(cfg), cluster.nodes, cluster.metrics, st, pod, cluster.now_ns, lo, hi)
    if not int(cfg[0]["fit_score"]):
        return kv
    fs = fit_scores(shape, cfg[0]["fit_resource_weights"][:2], cluster.nodes["allocatable"][lo:hi, :2],
                    st["nonzero"][lo:hi], nonzero_request(cfg, pod))
    add = (fs * int(cfg[0]["weight_fit"])).astype(np.uint64) << np.uint64(32)
    return np.where(kv != 0, kv + add, kv).astype(np.uint64)


def _keys_fn(shape):
    """shape → keys(cfg, cluster, st, pod, lo, hi); a strategy name (fit_strategy_reference.LEAST / MOST) selects that
    file's keys, so one queue can be continued under either"""
    if isinstance(shape, str):
        return lambda cfg, cl, st, pod, lo=0, hi=None: S.keys(cfg, cl, st, pod, shape, lo, hi)
    return lambda cfg, cl, st, pod, lo=0, hi=None: keys(cfg, cl, st, pod, shape, lo, hi)


def schedule(cfg, cluster, pods, shape, quotas=None, st=None, batches=()) -> Result:
    """FIFO scheduling of `pods` under `shape` (fit_strategy_reference.schedule with the other Fit term); st / quotas
    given are continued from (st in place)"""
    kf = _keys_fn(shape)
    pods = np.ascontiguousarray(pods, dtype=abi.POD_DTYPE)
    st = initial_states(cfg, cluster) if st is None else st
    quotas = None if quotas is None else quotas.copy()
    n = len(pods)
    node, score = np.full(n, -1, np.int32), np.zeros(n, np.int64)
    lead = np.full((len(batches), n), -1, np.int32)
    snaps = [None] * len(batches)
    for j in range(n):
        pod = pods[j:j + 1]
        for b, size in enumerate(batches):
            if j % size == 0:
                snaps[b] = st.copy()
            top = int(kf(cfg, cluster, snaps[b], pod).max(initial=0))
            lead[b, j] = key_node(top) if top else -1
        qid = int(pod["quota_id"][0])
        if quotas is not None and qid > 0 and not oracle.quota_admit(quotas[qid - 1], pod):
            continue
        best = int(kf(cfg, cluster, st, pod).max(initial=0))
        if best == 0:
            continue
        w = key_node(best)
        oracle.apply_pod(cfg, st, pod, w)
        if quotas is not None and qid > 0:
            oracle.quota_charge(quotas, qid - 1, pod)
        node[j], score[j] = w, best >> 32
    return Result(node, score, st, quotas, lead)


def records(cfg, cluster, snap_st, pods, shape, kc: int = KC):
    """per pod (the kc largest keys on the snapshot, descending, and a strict bound on the keys left out)"""
    kf, out = _keys_fn(shape), []
    for j in range(len(pods)):
        kv = np.sort(kf(cfg, cluster, snap_st, pods[j:j + 1]))[::-1]
        kv = [int(k) for k in kv if k]
        out.append((kv[:kc], kv[kc] + 1 if len(kv) > kc else 0))
    return out


def sequential_answer(cfg, cluster, snap_st, pods, prev=(), shape=RISING):
    """→ (keys of the round's pods, the winners in order, the state): the pods replayed on snapshot + the earlier rounds'
    placements prev = [[(pod record, node), ...], ...]"""
    kf, st = _keys_fn(shape), snap_st.copy()
    for lst in prev:
        for pod, nd in lst:
            oracle.apply_pod(cfg, st, pod, int(nd))
    out, published = [], []
    for j in range(len(pods)):
        best = int(kf(cfg, cluster, st, pods[j:j + 1]).max(initial=0))
        out.append(best)
        if best:
            oracle.apply_pod(cfg, st, pods[j:j + 1], key_node(best))
            published.append(key_node(best))
    return out, published, st


def skip_rule_answer(cfg, cluster, snap_st, pods, prev=(), shape=RISING, recs=None, kc: int = KC, bank: int = BANK,
                     probe: int = PROBE):
    """The keys a resolver keeping the monotone rule would give; it stops where its best answer lies below the record's
    bound, as the resolver does."""
    kf = _keys_fn(shape)
    recs = records(cfg, cluster, snap_st, pods, shape, kc) if recs is None else recs
    st = snap_st.copy()
    slot_of, n_slots = {}, 0
    for lst in prev:
        for pod, nd in lst:
            oracle.apply_pod(cfg, st, pod, int(nd))
            slot_of.setdefault(int(nd), n_slots)
            n_slots += 1
    out = []
    for j in range(len(pods)):
        pod = pods[j:j + 1]
        listed, ub = recs[j]
        pos = next((i for i, k in enumerate(listed) if key_node(k) not in slot_of), kc)
        best = listed[pos] if pos < len(listed) else 0
        if n_slots > 0 and pos > 0:
            need1 = n_slots > bank
            if need1 and pos <= probe:
                need1 = any(slot_of.get(key_node(k), -1) >= bank for k in listed[:pos])
            for m, s in slot_of.items():
                if s < bank or need1:
                    best = max(best, int(kf(cfg, cluster, st, pod, m, m + 1)[0]))
        if best < ub:
            break
        out.append(best)
        if best:
            w = key_node(best)
            oracle.apply_pod(cfg, st, pod, w)
            if w not in slot_of:
                slot_of[w] = n_slots
                n_slots += 1
    return out
