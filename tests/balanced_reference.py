"""Plain model of NodeResourcesBalancedAllocation next to NodeResourcesFit / LoadAwareScheduling on top of the committed
oracle — TEST INFRASTRUCTURE.  It follows tests/fit_strategy_reference.py step for step and uses its
helpers.  Per pod, in FIFO order:

  1. oracle.node_keys: every Filter's verdict and the Fit + LoadAware part of the total on the current state (the
     function knows nothing of the upstream default plugins);
  2. weight_balanced x the Balanced score is added to every non-zero key.  The score is oracle.balanced_score's rule on
     the row's Allocatable, st["requested"] (Requested, not NonZeroRequested) and the pod's plain requests;
  3. the largest key wins, ties on the lowest node index;
  4. the winner is applied with oracle.apply_pod;
  5. with quotas: oracle.quota_admit before the search, oracle.quota_charge on placement.

`balanced_scores` is the rule over all nodes in numpy float64 (IEEE binary64, round to nearest, like Go's float64 and the
oracle's C double); tests/test_balanced_rule.py holds it equal to oracle.balanced_score row by row, and holds `schedule`
equal to oracle.schedule_resv(cfg, ..., rsv=None, preds=zero rows) — the anchor that makes the model more than a
restatement.

`skip_rule_answer` is NOT the model: it is what the round engine's resolver would answer had it kept the monotone rule of
DESIGN.md §3.3 under this profile."""
from __future__ import annotations

import numpy as np

import fit_strategy_reference as S
from fit_strategy_reference import KC, BANK, PROBE, Result, initial_states, key_node, make_key  # noqa: F401
from koordinator_amd import abi
from oracle import oracle


def balanced_scores(alloc, requested, pod_req, resources: int = 3) -> np.ndarray:
    """oracle.balanced_score over every node: alloc, requested int64[n, 2] (cpu, memory), pod_req (cpu, memory)"""
    alloc = np.asarray(alloc, dtype=np.int64)
    total = np.asarray(requested, dtype=np.int64) + np.asarray(pod_req, dtype=np.int64)[None, :]
    n = len(alloc)
    fr, part = [], []
    for r in range(2):
        on = (alloc[:, r] != 0) if (resources >> r) & 1 else np.zeros(n, dtype=bool)
        f = total[:, r].astype(np.float64) / np.where(on, alloc[:, r], 1).astype(np.float64)
        fr.append(np.minimum(f, 1.0))  # (no NaN: the divisor is never 0)
        part.append(on)
    std = np.where(part[0] & part[1], np.abs((fr[0] - fr[1]) / 2.0), 0.0)
    return ((1.0 - std) * 100.0).astype(np.int64)  # int64(): truncation, the value is in [50, 100]


def pod_request(pod) -> tuple:
    return int(pod["requests"][0, abi.RES_CPU]), int(pod["requests"][0, abi.RES_MEMORY])


def keys(cfg, cluster, st, pod, lo: int = 0, hi: int | None = None) -> np.ndarray:
    """packed keys of `pod` on nodes [lo, hi) of the current state (steps 1 and 2)"""
    hi = cluster.n if hi is None else hi
    pod = np.asarray(pod, dtype=abi.POD_DTYPE).reshape(1)
    kv = oracle.node_keys(cfg, cluster.nodes, cluster.metrics, st, pod, cluster.now_ns, lo, hi)
    c = cfg[0]
    if not int(c["balanced_score"]):
        return kv
    cols = [abi.RES_CPU, abi.RES_MEMORY]
    bs = balanced_scores(cluster.nodes["allocatable"][lo:hi][:, cols], st["requested"][lo:hi][:, cols], pod_request(pod),
                         int(c["balanced_resources"]))
    add = (bs * int(c["weight_balanced"])).astype(np.uint64) << np.uint64(32)
    return np.where(kv != 0, kv + add, kv).astype(np.uint64)


def schedule(cfg, cluster, pods, quotas=None, st=None, batches=()) -> Result:
    """FIFO scheduling of `pods`; fit_strategy_reference.schedule with this module's keys"""
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
            top = int(keys(cfg, cluster, snaps[b], pod).max(initial=0))
            lead[b, j] = key_node(top) if top else -1
        qid = int(pod["quota_id"][0])
        if quotas is not None and qid > 0 and not oracle.quota_admit(quotas[qid - 1], pod):
            continue
        best = int(keys(cfg, cluster, st, pod).max(initial=0))
        if best == 0:
            continue
        w = key_node(best)
        oracle.apply_pod(cfg, st, pod, w)
        if quotas is not None and qid > 0:
            oracle.quota_charge(quotas, qid - 1, pod)
        node[j], score[j] = w, best >> 32
    return Result(node, score, st, quotas, lead)


def oracle_schedule(cfg, cluster, pods, quotas=None):
    """oracle.schedule_resv without reservations and with all-zero predicate rows → (node, score, state, quotas)"""
    st = initial_states(cfg, cluster)
    quotas = None if quotas is None else quotas.copy()
    preds = np.zeros(cluster.n, dtype=abi.NODE_PRED_DTYPE)
    node, score, _ = oracle.schedule_resv(cfg, cluster.nodes, cluster.metrics, st, None, pods, cluster.now_ns,
                                          quotas=quotas, n_threads=8, preds=preds)
    return node, score, st, quotas


def records(cfg, cluster, snap_st, pods, kc: int = KC):
    """per pod (the kc largest keys on the snapshot, descending, and a strict bound on the keys left out)"""
    out = []
    for j in range(len(pods)):
        kv = np.sort(keys(cfg, cluster, snap_st, pods[j:j + 1]))[::-1]
        kv = [int(k) for k in kv if k]
        out.append((kv[:kc], kv[kc] + 1 if len(kv) > kc else 0))
    return out


def sequential_answer(cfg, cluster, snap_st, pods, prev=()):
    """→ (keys of the round's pods, the winners in order, the state): the pods replayed on snapshot + the earlier rounds'
    placements prev = [[(pod record, node), ...], ...]"""
    st = snap_st.copy()
    for lst in prev:
        for pod, nd in lst:
            oracle.apply_pod(cfg, st, pod, int(nd))
    out, published = [], []
    for j in range(len(pods)):
        best = int(keys(cfg, cluster, st, pods[j:j + 1]).max(initial=0))
        out.append(best)
        if best:
            oracle.apply_pod(cfg, st, pods[j:j + 1], key_node(best))
            published.append(key_node(best))
    return out, published, st


def skip_rule_answer(cfg, cluster, snap_st, pods, prev=(), recs=None, kc: int = KC, bank: int = BANK,
                     probe: int = PROBE):
    """The keys a resolver keeping the monotone rule would give (fit_strategy_reference.skip_rule_answer on this
    module's keys)."""
    recs = records(cfg, cluster, snap_st, pods, kc) if recs is None else recs
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
                    best = max(best, int(keys(cfg, cluster, st, pod, m, m + 1)[0]))
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
