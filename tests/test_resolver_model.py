"""The resolver's plain model, its checker and its scenarios, on the CPU (DESIGN.md §4 "The resolver, branch by
branch"; the GPU side is tests/test_resolver_branches.py).

  * every scenario of tests/resolver_scenarios.py, on records from tests/round_model.py (whose keys >= ub and whose ub
    equal the device's by tests/test_round_records.py): the model's census contains the branch the scenario is named
    after, the replay agrees with the full sequential oracle, and the checker accepts the model's own answer;
  * the census of all scenarios together covers every branch of the list — the coverage condition, checked before a
    GPU is involved;
  * the checker is tested as tests/test_round_checks.py tests the record checkers: start from a correct result, apply
    one fault a resolver could make, and the checker must reject it."""
import numpy as np
import pytest

import resolver_model as RM
import resolver_scenarios as S
from oracle import oracle
from round_checks import CheckFailed, key_node

# the issue's list of branches, by census tag; S.BRANCHES (what the scenarios claim) must cover it
REQUIRED = {
    "fast", "fast-empty", "slow-e-wins", "slow-touched-wins", "win-bank0", "win-bank1", "tie-touched", "tie-cross-bank",
    "last_w-fresh", "last_w-touched", "pend-staged", "pend-hbm", "pend-never", "pend-rewin-twice",
    "prev-total-63", "prev-total-64", "prev-total-65", "prev-total-96", "slot-63", "slot-64", "slot-127",
    "probe-hit", "probe-miss", "probe-past", "dup-in-list", "dup-across-lists", "empty-list-between",
    "stop-at-0", "stop-middle", "stop-last", "best-eq-ub", "unschedulable", "unsched-inside", "shared-winner-3",
    "quota-reject", "quota-exhausted-in-round", "aux-reject-table", "aux-reject-round", "over-capacity-touched", "stale",
}
_tables = {}


def bench(name, bits):
    table, kw, build, tags = S.SCENARIOS[name]
    if table not in _tables:
        _tables[table] = S.make_table(table)
    cl, pods, quotas = _tables[table]
    return S.Bench(S._cfg(weights=S.WIDTHS[bits], **kw), cl, pods, quotas), build, tags


def as_device(sit, rp):
    """What kg_debug_resolve + read_state + read_quotas would return for a resolver that answers as the model does."""
    return {"consumed": rp.consumed, "cursor": rp.cursor, "poison": rp.poison, "rounds": rp.rounds, "error": 0,
            "slow": rp.slow, "out_keys": np.array(rp.out_keys, dtype=np.uint64), "list": list(rp.published),
            "state": RM.model_state(rp.st), "quotas": rp.quotas}


def cases():
    return [pytest.param(n, b, id=f"{n}-bits{b}") for n, s in S.SCENARIOS.items() for b in S.WIDTHS
            if b == 13 or not ({"profile", "la"} & set(s[1]))]


_census = {}


@pytest.mark.parametrize("name,bits", cases())
def test_scenario_selects_its_branch(name, bits):
    b, build, tags = bench(name, bits)
    sit = build(b)
    rp = RM.replay(sit, b.records(sit.first, sit.nb), b.consts["kc"])
    got = RM.all_tags(*RM.census(sit, rp, b.consts))
    _census[(name, bits)] = got
    assert tags <= got, f"{name}: the census lacks {sorted(tags - got)}: {sorted(got)}"
    RM.check(as_device(sit, rp), rp, name)
    RM.check_sequential(sit, rp.out_keys, rp.consumed, name)


def test_scenarios_cover_every_branch():
    assert REQUIRED <= S.BRANCHES, sorted(REQUIRED - S.BRANCHES)
    for bits in S.WIDTHS:
        got = set()
        for name, s in S.SCENARIOS.items():
            if bits == 14 and ({"profile", "la"} & set(s[1])):
                continue
            if (name, bits) not in _census:  # run alone: build it here
                b, build, _ = bench(name, bits)
                sit = build(b)
                rp = RM.replay(sit, b.records(sit.first, sit.nb), b.consts["kc"])
                _census[(name, bits)] = RM.all_tags(*RM.census(sit, rp, b.consts))
            got |= _census[(name, bits)]
        missing = REQUIRED - got - ({"over-capacity-touched"} if bits == 14 else set())  # (that profile runs at one width)
        assert not missing, f"score_bits {bits}: no scenario selects {sorted(missing)}"


# ---- the checker rejects what a faulty resolver would answer ----------------------------------------------------
def faulty_resolver(sit, records, consts, fault):
    """The replay rule with one fault a resolver could make (names below); → the device dict of that resolver."""
    kc = consts["kc"]
    st = sit.st0.copy()
    for lst in sit.prev:
        for pi, nd in lst:
            oracle.apply_pod(sit.cfg, st, sit.pods[pi], int(nd), +1)
    n_slots = sum(len(l) for l in sit.prev)
    slot_of = {}
    for s, nd in enumerate(int(nd) for lst in sit.prev for _, nd in lst):
        slot_of.setdefault(nd, s)
    st_eval = st.copy()  # what the resolver's rows hold (a never-assumed pending row lags the table)
    quotas = None if sit.quotas is None else sit.quotas.copy()
    out, published, winners = [RM.SENTINEL] * sit.nb, [], []
    consumed = slow = 0
    last_fresh = None
    true_stop = RM.replay(sit, records, kc).consumed
    for j in range(sit.nb):
        pod = sit.pods[sit.first + j]
        listed = [int(k) for k in records[j][:kc] if k]
        ub = int(records[j][kc])
        qid = int(pod["quota_id"])
        if quotas is not None and qid > 0 and not oracle.quota_admit(quotas[qid - 1], pod):
            if fault == "quota-charged-rejected":
                oracle.quota_charge(quotas, qid - 1, pod)
            out[j] = 0
            consumed += 1
            continue
        tset = set(slot_of)
        if fault == "last_w-missing" and last_fresh is not None:
            tset.discard(last_fresh)
        pos = next((i for i, k in enumerate(listed) if key_node(k) not in tset), kc)
        slow += bool(slot_of) and pos > 0
        ebest = max((k for k in listed if k >= ub and key_node(k) not in tset), default=0)
        rows = [m for m in tset if not (fault == "bank1-ignored" and slot_of[m] >= RM.BANK)]
        tk = {m: RM.key_now(sit, st_eval, pod, m) for m in rows}
        mbest = max(tk.values(), default=0)
        if fault == "tie-higher-index" and mbest:
            mbest = min(k for k in tk.values() if k >> 32 == mbest >> 32)
        best = max(ebest, mbest)
        stop_here = best < ub
        if fault == "stop-early":
            stop_here = j == true_stop - 1 or stop_here
        if fault == "stop-late" and j == true_stop:
            stop_here = False
        if stop_here:
            if fault == "writeback-past-consumed" and best:
                winners.append((pod, key_node(best)))
            break
        out[j] = best
        consumed += 1
        last_fresh = None
        if best:
            w = key_node(best)
            fresh = w not in slot_of
            winners.append((pod, w))
            published.append(w)
            if quotas is not None and qid > 0:
                oracle.quota_charge(quotas, qid - 1, pod)
            if not (fresh and fault == "pending-never-assumed"):
                oracle.apply_pod(sit.cfg, st_eval, pod, w, +1)
            if fresh:
                slot_of[w] = n_slots
                n_slots += 1
                last_fresh = w
    seen = set()
    for pod, w in winners:  # the write-back
        if fault == "shared-winner-once" and w in seen:
            continue
        seen.add(w)
        oracle.apply_pod(sit.cfg, st, pod, w, +1)
    return {"consumed": consumed, "cursor": sit.first + consumed, "poison": int(consumed < sit.nb), "rounds": 1,
            "error": 0, "slow": slow + (fault == "slow-off-by-one"), "out_keys": np.array(out, dtype=np.uint64),
            "list": published, "state": RM.model_state(st), "quotas": quotas}


# fault → (a scenario whose branch the fault breaks, the rules that may catch it)
FAULTS = {
    "bank1-ignored": ("touched-wins-bank1", {"out-keys"}),
    "last_w-missing": ("last_w-fresh", {"out-keys"}),
    "pending-never-assumed": ("last_w-fresh", {"out-keys"}),
    "tie-higher-index": ("tie-same-bank", {"out-keys"}),
    "stop-early": ("stop-middle", {"consumed"}),
    "stop-late": ("stop-middle", {"consumed"}),
    "writeback-past-consumed": ("stop-middle", {"state"}),
    "shared-winner-once": ("pend-rewin-shared", {"state"}),
    "quota-charged-rejected": ("quota", {"quota"}),
    "slow-off-by-one": ("slow-e-wins", {"slow"}),
}


@pytest.mark.parametrize("bits", list(S.WIDTHS))
def test_faultless_resolver_is_accepted(bits):
    for name in sorted({s for s, _ in FAULTS.values()}):
        b, build, _ = bench(name, bits)
        sit = build(b)
        recs = b.records(sit.first, sit.nb)
        RM.check(faulty_resolver(sit, recs, b.consts, None), RM.replay(sit, recs, b.consts["kc"]), name)


@pytest.mark.parametrize("fault", list(FAULTS))
def test_checker_rejects_fault(fault):
    name, rules = FAULTS[fault]
    b, build, _ = bench(name, 13)
    sit = build(b)
    recs = b.records(sit.first, sit.nb)
    dev = faulty_resolver(sit, recs, b.consts, fault)
    with pytest.raises(CheckFailed) as err:
        RM.check(dev, RM.replay(sit, recs, b.consts["kc"]), f"{name} with {fault}")
    assert err.value.rule in rules, (fault, err.value.rule, str(err.value))
