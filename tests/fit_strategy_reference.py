"""Plain model of NodeResourcesFit's scoring strategies on top of the committed oracle (kg_config.fit_scoring_strategy,
DESIGN.md §3.24) — TEST INFRASTRUCTURE.  The oracle scores Fit by LeastAllocated only and stays as it is; the
MostAllocated rule is upstream v1.24's mostResourceScorer, restated as published:

  each resource (cpu, memory) takes part when its weight and the node's allocatable are non-zero;
  q = min(NonZeroRequested_node + NonZeroRequest_pod, allocatable) * 100 // allocatable  (over-committed: 100);
  score = sum(q * w) // sum(w), 0 when no resource takes part.

Per pod, in FIFO order:
  1. oracle.node_keys with a copy of the config whose fit_score is 0: every Filter's verdict and LoadAware's part of the
     total on the current state;
  2. weight_fit x the Fit score is added to every non-zero key.  The pod's non-zero request is what oracle.apply_pod
     adds to a zeroed state row;
  3. the largest key wins, ties on the lowest node index (the packed key's low word);
  4. the winner is applied with oracle.apply_pod;
  5. with quotas: oracle.quota_admit before the search, oracle.quota_charge on placement.

`fit_score` is the rule in Python integers, one row at a time — the definition, and what the known answers are checked
against.  `fit_scores` is the same arithmetic over all nodes in int64 (every product is asserted to stay below 2^62);
tests/test_fit_strategy_rule.py holds the two equal.

`skip_rule_answer` is NOT the model: it is what the round engine's resolver would answer had it kept the monotone rule of
DESIGN.md §3.3 under MostAllocated (modified rows re-scored only when one of them is listed above the best unmodified
candidate; the second register bank only when one of its rows is among the first few listed keys).  The tests use it to
show that a scenario tells the two rules apart."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from koordinator_amd import abi
from oracle import oracle

LEAST, MOST = "LeastAllocated", "MostAllocated"
KC, BANK, PROBE = 64, 64, 8  # candidates per record, modified-row slots per register bank, bank-1 probe length


def make_key(total: int, node: int) -> int:
    return (int(total) << 32) | (0xFFFFFFFF - int(node))


def key_node(key: int) -> int:
    return 0xFFFFFFFF - (int(key) & 0xFFFFFFFF)


def nonzero_request(cfg, pod) -> tuple:
    """(cpu, memory) NodeInfo.AddPod adds to NonZeroRequested for `pod`: read off a zeroed state row"""
    row = oracle.states(1)
    oracle.apply_pod(cfg, row, pod, 0)
    return int(row["nonzero"][0, 0]), int(row["nonzero"][0, 1])


def fit_score(strategy: str, weights, alloc, nz_node, nz_pod) -> int:
    """NodeResourcesFit Score of one row in Python integers; weights / alloc / nz_node / nz_pod: (cpu, memory)"""
    s = ws = 0
    for r in range(2):
        w, cap = int(weights[r]), int(alloc[r])
        if w == 0 or cap == 0:
            continue
        req = int(nz_node[r]) + int(nz_pod[r])
        if strategy == MOST:
            q = min(req, cap) * 100 // cap
        else:
            q = 0 if req > cap else (cap - req) * 100 // cap
        s += q * w
        ws += w
    return s // ws if ws else 0


def fit_scores(strategy: str, weights, alloc, nz_node, nz_pod) -> np.ndarray:
    """fit_score over every node: alloc, nz_node int64[n, 2] → int64[n]"""
    alloc = np.asarray(alloc, dtype=np.int64)
    req = np.asarray(nz_node, dtype=np.int64) + np.asarray(nz_pod, dtype=np.int64)[None, :]
    assert (alloc >= 0).all() and (req >= 0).all() and int(alloc.max(initial=0)) < 1 << 55 and int(req.max(initial=0)) < 1 << 55
    s = np.zeros(len(alloc), dtype=np.int64)
    ws = np.zeros(len(alloc), dtype=np.int64)
    for r in range(2):
        w = int(weights[r])
        cap = alloc[:, r]
        part = (cap != 0) if w else np.zeros(len(alloc), dtype=bool)
        safe = np.where(cap != 0, cap, 1)
        if strategy == MOST:
            q = np.minimum(req[:, r], cap) * 100 // safe
        else:
            q = np.where(req[:, r] > cap, 0, (cap - req[:, r]) * 100 // safe)
        s += np.where(part, q * w, 0)
        ws += np.where(part, w, 0)
    return np.where(ws != 0, s // np.where(ws != 0, ws, 1), 0)


def _cfg_no_fit_score(cfg):
    c = cfg.copy()
    c["fit_score"] = 0
    return c


def keys(cfg, cluster, st, pod, strategy: str, lo: int = 0, hi: int | None = None) -> np.ndarray:
    """packed keys of `pod` on nodes [lo, hi) of the current state under `strategy` (steps 1 and 2)"""
    hi = cluster.n if hi is None else hi
    kv = oracle.node_keys(_cfg_no_fit_score(cfg), cluster.nodes, cluster.metrics, st, pod, cluster.now_ns, lo, hi)
    if not int(cfg[0]["fit_score"]):
        return kv
    fs = fit_scores(strategy, cfg[0]["fit_resource_weights"][:2], cluster.nodes["allocatable"][lo:hi, :2],
                    st["nonzero"][lo:hi], nonzero_request(cfg, pod))
    add = (fs * int(cfg[0]["weight_fit"])).astype(np.uint64) << np.uint64(32)
    return np.where(kv != 0, kv + add, kv).astype(np.uint64)


def initial_states(cfg, cluster):
    st = oracle.states(cluster.n)
    if len(cluster.existing_pods):
        oracle.add_pods(cfg, st, cluster.existing_pods, cluster.existing_node)
    return st


@dataclass
class Result:
    node: np.ndarray      # int32[n], -1 = unschedulable
    score: np.ndarray     # int64[n], the winner's weighted total
    st: np.ndarray        # the oracle state after the queue
    quotas: np.ndarray | None
    lead: np.ndarray      # int32[len(batches), n]: the node leading the pod's round-start keys (-1 none)


def schedule(cfg, cluster, pods, strategy: str = MOST, quotas=None, st=None, batches=()) -> Result:
    """FIFO scheduling of `pods` under `strategy`.  batches: for each batch size b, lead[b's position][j] = the node that
    leads pod j's keys on the state at the start of its group of b pods (what a round's wide pass would see)."""
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
            top = int(keys(cfg, cluster, snaps[b], pod, strategy).max(initial=0))
            lead[b, j] = key_node(top) if top else -1
        qid = int(pod["quota_id"][0])
        if quotas is not None and qid > 0 and not oracle.quota_admit(quotas[qid - 1], pod):
            continue
        best = int(keys(cfg, cluster, st, pod, strategy).max(initial=0))
        if best == 0:
            continue
        w = key_node(best)
        oracle.apply_pod(cfg, st, pod, w)
        if quotas is not None and qid > 0:
            oracle.quota_charge(quotas, qid - 1, pod)
        node[j], score[j] = w, best >> 32
    return Result(node, score, st, quotas, lead)


def records(cfg, cluster, snap_st, pods, strategy: str, kc: int = KC):
    """per pod (the kc largest keys on the snapshot, descending, and a strict bound on the keys left out)"""
    out = []
    for j in range(len(pods)):
        kv = np.sort(keys(cfg, cluster, snap_st, pods[j:j + 1], strategy))[::-1]
        kv = [int(k) for k in kv if k]
        out.append((kv[:kc], kv[kc] + 1 if len(kv) > kc else 0))
    return out


def sequential_answer(cfg, cluster, snap_st, pods, prev=(), strategy: str = MOST):
    """→ (keys of the round's pods, the winners in order, the state): the pods replayed on snapshot + the earlier rounds'
    placements prev = [[(pod record, node), ...], ...]"""
    st = snap_st.copy()
    for lst in prev:
        for pod, nd in lst:
            oracle.apply_pod(cfg, st, pod, int(nd))
    out, published = [], []
    for j in range(len(pods)):
        best = int(keys(cfg, cluster, st, pods[j:j + 1], strategy).max(initial=0))
        out.append(best)
        if best:
            oracle.apply_pod(cfg, st, pods[j:j + 1], key_node(best))
            published.append(key_node(best))
    return out, published, st


def skip_rule_answer(cfg, cluster, snap_st, pods, prev=(), strategy: str = MOST, recs=None, kc: int = KC,
                     bank: int = BANK, probe: int = PROBE):
    """The keys a resolver keeping the monotone rule would give (see the module text); it stops where its best answer
    lies below the record's bound, as the resolver does.  recs: the round's records, default the snapshot's."""
    recs = records(cfg, cluster, snap_st, pods, strategy, kc) if recs is None else recs
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
                    best = max(best, int(keys(cfg, cluster, st, pod, strategy, m, m + 1)[0]))
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
