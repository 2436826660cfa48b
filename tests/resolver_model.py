"""A plain model of the round engine's resolver (DESIGN.md §3.3, §4 "The resolver, branch by branch") — TEST
INFRASTRUCTURE.

`replay` is §3.3's exactness argument written as code: given the records the resolver consumed, the cluster, the
earlier rounds' placements and the pods, it replays the pods in order on an oracle state that starts at snapshot +
interventions.  For pod j, best = the largest of {listed keys >= ub_j whose node nobody has touched since the snapshot}
∪ {exact current keys of every touched node}; the round stops before j iff best < ub_j; best == 0 with ub_j == 0 is
"unschedulable".  Listed keys below ub are ignored (the device may differ there, and they cannot change
the outcome).  It knows nothing of register banks, bitmaps or hashes.

`census` names, per pod and per round, which of the resolver's branches the situation selects.  It is derived from
the record and the replay, with the geometry constants the device reports (slots per bank, staged rows, probe length),
never from what the device answered.

`check` compares what kg_debug_resolve returned with the replay; `check_sequential` compares every consumed pod's key
with the full sequential oracle on the evolving state, with no reference to the record.  A failed check raises
round_checks.CheckFailed, which names the rule broken (`.rule`)."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from koordinator_amd import abi
from oracle import oracle
from round_checks import CheckFailed, key_node

SENTINEL = abi.DBG_RESOLVE_SENTINEL
BANK = 64  # modified-row slots per register bank: the resolver's wave width
STATE_COLUMNS = (("requested_cpu", "requested", abi.RES_CPU), ("requested_mem", "requested", abi.RES_MEMORY),
                 ("nonzero_cpu", "nonzero", 0), ("nonzero_mem", "nonzero", 1), ("num_pods", "num_pods", None),
                 ("la_est_cpu", "la_est_all", 0), ("la_est_mem", "la_est_all", 1),
                 ("la_est_prod_cpu", "la_est_prod", 0), ("la_est_prod_mem", "la_est_prod", 1))


@dataclass
class Situation:
    cfg: np.ndarray
    cl: object                    # synth.Cluster
    st0: np.ndarray               # the oracle state the wide pass read: the snapshot
    pods: np.ndarray              # the staged queue
    first: int
    nb: int
    prev: list = field(default_factory=list)  # prev[0] = the round just before: [(staged pod index, node), ...]
    quotas: np.ndarray | None = None
    poison: bool = False
    cursor: int | None = None


@dataclass
class Replay:
    out_keys: list
    consumed: int
    rounds: int
    cursor: int
    poison: int
    slow: int
    published: list
    st_pre: np.ndarray            # snapshot + interventions
    st: np.ndarray                # ... + this round's write-back
    quotas: np.ndarray | None
    trace: list                   # one dict per pod looked at (the stopped pod included)


def key_now(sit: Situation, st, pod, node: int) -> int:
    cl = sit.cl
    return int(oracle.node_keys(sit.cfg, cl.nodes, cl.metrics, st, pod, cl.now_ns, node, node + 1)[0])


def replay(sit: Situation, records: np.ndarray, kc: int) -> Replay:
    st = sit.st0.copy()
    touched, tset = [], set()
    for lst in sit.prev:
        for pi, nd in lst:
            oracle.apply_pod(sit.cfg, st, sit.pods[pi], int(nd), +1)
            if nd not in tset:
                tset.add(int(nd))
                touched.append(int(nd))
    st_pre = st.copy()
    quotas = None if sit.quotas is None else sit.quotas.copy()
    out = [SENTINEL] * sit.nb
    if sit.poison or (sit.cursor is not None and sit.cursor != sit.first):  # a stale round: only the sequence word moves
        return Replay(out, 0, 0, sit.first if sit.cursor is None else sit.cursor, int(sit.poison), 0, [], st_pre, st,
                      quotas, [])
    trace, slow, consumed, published = [], 0, 0, []
    for j in range(sit.nb):
        pod = sit.pods[sit.first + j]
        listed = [int(k) for k in records[j][:kc] if k]
        ub = int(records[j][kc])
        t = {"j": j, "ub": ub, "listed": listed, "touched": list(touched), "rejected": False, "stopped": False,
             "winner": None, "from_touched": False, "best": 0, "tkeys": {}}
        trace.append(t)
        qid = int(pod["quota_id"])
        if quotas is not None and qid > 0 and not oracle.quota_admit(quotas[qid - 1], pod):
            t["rejected"] = True  # PreFilter Unschedulable: consumed, not placed, not charged
            out[j] = 0
            consumed += 1
            continue
        t["pos"] = next((i for i, k in enumerate(listed) if key_node(k) not in tset), kc)
        t["slow"] = bool(touched) and t["pos"] > 0
        slow += t["slow"]
        t["tkeys"] = {m: key_now(sit, st, pod, m) for m in touched}
        ebest = max((k for k in listed if k >= ub and key_node(k) not in tset), default=0)
        mbest = max(t["tkeys"].values(), default=0)
        best = t["best"] = max(ebest, mbest)
        if best < ub:
            t["stopped"] = True
            break
        out[j] = best
        consumed += 1
        if best:
            w = t["winner"] = key_node(best)
            t["from_touched"] = w in tset
            oracle.apply_pod(sit.cfg, st, pod, w, +1)
            if quotas is not None and qid > 0:
                oracle.quota_charge(quotas, qid - 1, pod)
            if w not in tset:
                tset.add(w)
                touched.append(w)
            published.append(w)
    return Replay(out, consumed, 1, sit.first + consumed, int(consumed < sit.nb), slow, published, st_pre, st, quotas,
                  trace)


# ---- the branch census ----------------------------------------------------------------------------------------------
def _aux_tags(sit, rp, t, st_before, round_placed):
    """A touched row that fits on cpu / memory but not on an aux resource: because of what the table holds, or only
    because of this round's earlier pods."""
    pod = sit.pods[sit.first + t["j"]]
    if not pod["requests"][abi.RES_CPU + 2:].any():
        return set()
    bare = pod.copy()
    bare["requests"][abi.RES_CPU + 2:] = 0
    tags = set()
    for m, k in t["tkeys"].items():
        if k != 0 or key_now(sit, st_before, bare, m) == 0:
            continue
        alt = st_before.copy()
        alt["requested"][m, abi.RES_CPU + 2:] = rp.st_pre["requested"][m, abi.RES_CPU + 2:]
        tags.add("aux-reject-round" if key_now(sit, alt, pod, m) != 0 and m in round_placed else "aux-reject-table")
    return tags


def census(sit: Situation, rp: Replay, consts: dict):
    """(per-pod list of tag sets, round tag set) for the replay `rp`; consts: kg_debug_resolve's constants."""
    kc, staged, probe = consts["kc"], consts["staged"], consts["bank1_probe"]
    concat = [int(nd) for lst in sit.prev for _, nd in lst]
    slot_of = {}
    for s, nd in enumerate(concat):
        slot_of.setdefault(nd, s)
    n_slots = len(concat)
    rnd = {f"prev-total-{n_slots}"}
    for lst in sit.prev:
        nds = [nd for _, nd in lst]
        if len(set(nds)) < len(nds):
            rnd.add("dup-in-list")
    sets = [set(nd for _, nd in lst) for lst in sit.prev]
    if any(sets[a] & sets[b] for a in range(len(sets)) for b in range(a + 1, len(sets))):
        rnd.add("dup-across-lists")
    if any(not sets[i] and sets[i - 1] and sets[i + 1] for i in range(1, len(sets) - 1)):
        rnd.add("empty-list-between")
    if not rp.trace:
        rnd.add("stale")
        return [], rnd
    per_pod, pend, fresh_wins, prev_t = [], {}, {}, None
    st = rp.st_pre.copy()
    round_placed = set()
    for t in rp.trace:
        tags = set()
        per_pod.append(tags)
        if t["rejected"]:
            tags.add("quota-reject")
            prev_t = t
            continue
        listed, pos = t["listed"], t["pos"]
        if prev_t is not None and prev_t["winner"] is not None and listed and key_node(listed[0]) == prev_t["winner"]:
            tags.add("last_w-touched" if prev_t["from_touched"] else "last_w-fresh")

        def settle(bank):
            for nd in [n for n, (b, _) in pend.items() if b == bank]:
                tags.add("pend-staged" if pend.pop(nd)[1] < staged else "pend-hbm")

        if n_slots == 0:
            tags.add("fast-empty")
        elif pos == 0:
            tags.add("fast")
        else:
            settle(0)
            need1 = n_slots > BANK
            if need1 and pos <= probe:
                need1 = any(slot_of.get(key_node(k), -1) >= BANK for k in listed[:pos])
                tags.add("probe-hit" if need1 else "probe-miss")
            elif need1:
                tags.add("probe-past")
            if need1:
                settle(1)
            tags |= _aux_tags(sit, rp, t, st, round_placed)
            if not sit.cfg["fit_filter"][0] and any(
                    st["nonzero"][m, 0] >= sit.cl.nodes["allocatable"][m, abi.RES_CPU] for m in t["touched"]):
                tags.add("over-capacity-touched")
            if not t["stopped"]:
                tags.add("slow-touched-wins" if t["from_touched"] else "slow-e-wins")
        if t["stopped"]:
            tags.add("stop")
            rnd.add("stop-at-0" if t["j"] == 0 else "stop-last" if t["j"] == sit.nb - 1 else "stop-middle")
            break
        if t["best"] == t["ub"] and t["ub"] != 0:
            tags.add("best-eq-ub")
        if t["best"] == 0:
            tags.add("unschedulable")
            if 0 < t["j"] < sit.nb - 1:
                tags.add("unsched-inside")
        w = t["winner"]
        if w is not None:
            if t["from_touched"]:
                tags.add(f"win-bank{slot_of[w] // BANK}")
                ties = [m for m, k in t["tkeys"].items() if k and k >> 32 == t["best"] >> 32]
                if len(ties) > 1:
                    tags.add("tie-touched")
                    if len({slot_of[m] // BANK for m in ties}) > 1:
                        tags.add("tie-cross-bank")
                if w in fresh_wins:
                    fresh_wins[w] += 1
                    if fresh_wins[w] == 2:
                        tags.add("pend-rewin-twice")
            else:
                slot_of[w] = n_slots
                pend[w] = (n_slots // BANK, pos)
                tags.add(f"slot-{n_slots}")
                n_slots += 1
                fresh_wins[w] = 0
            oracle.apply_pod(sit.cfg, st, sit.pods[sit.first + t["j"]], w, +1)
            round_placed.add(w)
        prev_t = t
    if pend:
        rnd.add("pend-never")
    if max((rp.published.count(w) for w in set(rp.published)), default=0) >= 3:
        rnd.add("shared-winner-3")
    if sit.quotas is not None:
        # a quota that admitted a pod of this round and, charged by this round's pods, rejects a later one
        charged = {int(sit.pods[sit.first + t["j"]]["quota_id"]) for t in rp.trace if t["winner"] is not None}
        for t in rp.trace:
            pod = sit.pods[sit.first + t["j"]]
            if t["rejected"] and int(pod["quota_id"]) in charged and oracle.quota_admit(
                    sit.quotas[int(pod["quota_id"]) - 1], pod):
                rnd.add("quota-exhausted-in-round")
    return per_pod, rnd


def all_tags(per_pod, rnd) -> set:
    return set(rnd).union(*per_pod) if per_pod else set(rnd)


# ---- the checker ----------------------------------------------------------------------------------------------------
def model_state(st) -> dict:
    return {name: (st[col] if idx is None else st[col][:, idx]).astype(np.int64) for name, col, idx in STATE_COLUMNS}


def check(dev: dict, rp: Replay, what: str = ""):
    """dev: kg_debug_resolve's dict plus 'state' (Engine.read_state) and, with quotas, 'quotas' (Engine.read_quotas)."""
    if dev["error"] != 0:
        raise CheckFailed("error", f"{what}: CTL_ERROR = {dev['error']}")
    for name, want in (("consumed", rp.consumed), ("cursor", rp.cursor), ("poison", rp.poison), ("rounds", rp.rounds)):
        if dev[name] != want:
            raise CheckFailed(name, f"{what}: {name} {dev[name]}, the model's {want}")
    got = [int(k) for k in dev["out_keys"]]
    for j in range(len(got)):
        if got[j] != rp.out_keys[j]:
            rule = "past-consumed" if j >= rp.consumed else "out-keys"
            raise CheckFailed(rule, f"{what}: pod {j}: key {hex(got[j])} (node {key_node(got[j])}), the model's "
                                    f"{hex(rp.out_keys[j])} (node {key_node(rp.out_keys[j])})")
    if [int(x) for x in dev["list"]] != rp.published:
        raise CheckFailed("list", f"{what}: published {list(dev['list'])}, the model's {rp.published}")
    want = model_state(rp.st)
    for name in want:
        bad = np.nonzero(dev["state"][name] != want[name])[0]
        if len(bad):
            i = int(bad[0])
            raise CheckFailed("state", f"{what}: {name}[{i}] = {int(dev['state'][name][i])}, the model's "
                                       f"{int(want[name][i])} ({len(bad)} nodes differ)")
    if rp.quotas is not None and not np.array_equal(dev["quotas"], rp.quotas):
        k = int(np.nonzero(dev["quotas"] != rp.quotas)[0][0])
        raise CheckFailed("quota", f"{what}: quota row {k}: {dev['quotas'][k]}, the model's {rp.quotas[k]}")
    if dev["slow"] != rp.slow:
        raise CheckFailed("slow", f"{what}: CTL_SLOW {dev['slow']}, the model's {rp.slow}")


def check_sequential(sit: Situation, dev_keys, consumed: int, what: str = ""):
    """Every consumed pod's key against the full sequential oracle on the evolving state: no record involved."""
    cl = sit.cl
    st = sit.st0.copy()
    for lst in sit.prev:
        for pi, nd in lst:
            oracle.apply_pod(sit.cfg, st, sit.pods[pi], int(nd), +1)
    quotas = None if sit.quotas is None else sit.quotas.copy()
    for j in range(consumed):
        pod = sit.pods[sit.first + j]
        qid = int(pod["quota_id"])
        if quotas is not None and qid > 0 and not oracle.quota_admit(quotas[qid - 1], pod):
            want = 0
        else:
            want = int(oracle.node_keys(sit.cfg, cl.nodes, cl.metrics, st, pod, cl.now_ns, 0, cl.n).max())
        if int(dev_keys[j]) != want:
            raise CheckFailed("sequential", f"{what}: pod {j}: key {hex(int(dev_keys[j]))} (node "
                                            f"{key_node(dev_keys[j])}), the sequential oracle's {hex(want)} (node "
                                            f"{key_node(want)})")
        if want:
            oracle.apply_pod(sit.cfg, st, pod, key_node(want), +1)
            if quotas is not None and qid > 0:
                oracle.quota_charge(quotas, qid - 1, pod)
