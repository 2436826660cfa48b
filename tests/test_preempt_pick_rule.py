"""The reference of kg_pods_pick_candidate (tests/pick_reference.py: upstream's pickOneNodeForPreemption as narrowing
passes) against hand-derived cases, one per rule where exactly that rule decides, and the binding's record layout."""
import os

import numpy as np

from koordinator_amd import abi
from pick_reference import pick_candidate


def arrays(cands):
    """[(reject, num_violating, [(kept, priority, start), ...]), ...] -> the arrays kg_pods_pick_candidate takes; node
    index of candidate c = 100 + c"""
    off = np.zeros(len(cands) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(v) for _, _, v in cands])
    flat = [t for _, _, v in cands for t in v]
    return (np.arange(100, 100 + len(cands), dtype=np.int32), off,
            np.array([r for r, _, _ in cands], dtype=np.int32),
            np.array([k for k, _, _ in flat], dtype=np.uint8),
            np.array([n for _, n, _ in cands], dtype=np.int32),
            np.array([p for _, p, _ in flat], dtype=np.int32),
            np.array([s for _, _, s in flat], dtype=np.int64))


def pick(cands):
    return pick_candidate(*arrays(cands))


def test_zero_victim_candidate_beats_everything():
    # candidate 1 fits once its only potential victim is reprieved (kept = 0): no preemption needed.  Candidate 0 is
    # better on every later rule's terms than anything with victims could be
    p = pick([(0, 0, [(1, -5, 9)]), (0, 0, [(0, 1000, 1)]), (0, 0, [(0, 7, 7)])])
    assert (p.candidate, p.node_idx, p.rule, p.victims, p.n_victims) == (1, 101, 0, [], 0)
    assert p.record() == (1, 101, 3, 0, 0, 0, 0, 0)


def test_violations_beat_priority():
    # candidate 0: one low-priority victim but a PDB violation; candidate 1: a high-priority victim, no violation
    p = pick([(0, 1, [(1, 0, 5)]), (0, 0, [(1, 1000, 5)])])
    assert (p.candidate, p.rule) == (1, 1)
    assert p.record() == (1, 101, 2, 1, 0, 1000, 1000 + 2**31, 5)


def test_first_victim_decides_not_the_maximum():
    # candidate 0's first kept victim is priority 10 but it holds a 1000 later; candidate 1's first is 500 (its
    # maximum).  Pods[0]: 10 < 500 → candidate 0, although its maximum (1000) is the higher one.  The reprieved entry in
    # front (kept = 0) is not Pods[0]
    p = pick([(0, 0, [(0, 900, 1), (1, 10, 1), (1, 1000, 1)]), (0, 0, [(1, 500, 1)])])
    assert (p.candidate, p.rule, p.victims, p.first_priority) == (0, 2, [1, 2], 10)


def test_sum_carries_the_offset_and_precedes_the_count():
    # "two victims at priority -1 lose to one at priority 10": behind a common first victim at -1, so that rule 2 ties.
    # [-1, -1, -1] sums to 3·2^31 - 3, [-1, 10] to 2·2^31 + 9.  Without the offset -3 < 9 and candidate 0 would win;
    # with it the list holding the 10 is the lower sum
    p = pick([(0, 0, [(1, -1, 1), (1, -1, 1), (1, -1, 1)]), (0, 0, [(1, -1, 1), (1, 10, 1)])])
    assert (p.candidate, p.rule, p.sum_priorities) == (1, 3, 2 * 2**31 + 9)
    # the sum is decided before the count: [0, INT32_MIN, INT32_MIN] sums to 2^31, [0, 5] to 2·2^31 + 5, so three
    # victims beat two
    lo = -2**31
    p = pick([(0, 0, [(1, 0, 1), (1, 5, 1)]), (0, 0, [(1, 0, 1), (1, lo, 1), (1, lo, 1)])])
    assert (p.candidate, p.rule, p.n_victims, p.sum_priorities) == (1, 3, 3, 2**31)


def test_first_victim_precedes_the_sum():
    # the same two lists without the common first victim: -1 < 10 on Pods[0], so rule 2 picks the two victims before
    # the sums are ever compared — upstream's order of the rules
    p = pick([(0, 0, [(1, -1, 1), (1, -1, 1)]), (0, 0, [(1, 10, 1)])])
    assert (p.candidate, p.rule) == (0, 2)


def test_count_decides():
    # equal violations, first priority and sum: [0, INT32_MIN] sums to 2^31 + 0 = [0]'s 2^31; one victim is fewer
    lo = -2**31
    p = pick([(0, 0, [(1, 0, 1), (1, lo, 1)]), (0, 0, [(1, 0, 1)])])
    assert (p.candidate, p.rule, p.n_victims) == (1, 4, 1)


def test_latest_earliest_start_decides_over_the_whole_list():
    # both: first priority 5, sum 2·2^31 + 105, two victims.  The maximum priority (100) sits second in both lists, so
    # the earliest start is that victim's: 30 against 40, not the first victims' 99 / 1.  Candidate 1's is later → wins
    p = pick([(0, 0, [(1, 5, 99), (1, 100, 30)]), (0, 0, [(1, 5, 1), (1, 100, 40)])])
    assert (p.candidate, p.rule, p.earliest_start_unix_nano) == (1, 5, 40)
    # several victims at the maximum: the earliest of them counts.  Candidate 0: max 7 at starts {50, 20} → 20;
    # candidate 1: max 7 at starts {25, 60} → 25, later → wins
    p = pick([(0, 0, [(1, 7, 50), (1, 7, 20)]), (0, 0, [(1, 7, 25), (1, 7, 60)])])
    assert (p.candidate, p.rule, p.earliest_start_unix_nano) == (1, 5, 25)


def test_full_tie_goes_to_the_lowest_position():
    same = [(1, 3, 10), (1, 3, 11)]
    p = pick([(1, 0, list(same)), (0, 0, list(same)), (0, 0, list(same))])
    assert (p.candidate, p.rule, p.eligible) == (1, 6, 2)


def test_no_eligible_candidate():
    p = pick([(abi.REJECT_FIT_CPU, 0, [(0, 1, 1)]), (abi.REJECT_NO_VICTIMS, 0, [])])
    assert p.record() == (-1, -1, 0, 0, 0, 0, 0, 0) and p.rule is None and p.victims == []
    assert pick([]).record() == (-1, -1, 0, 0, 0, 0, 0, 0)


def test_single_candidate_returns_at_rule_one():
    p = pick([(0, 2, [(1, 4, 8)])])
    assert (p.candidate, p.rule) == (0, 1)
    assert p.record() == (0, 100, 1, 1, 2, 4, 4 + 2**31, 8)


def test_record_layout():
    assert abi.PREEMPT_PICK_DTYPE.itemsize == 64
    assert abi.PREEMPT_PICK_DTYPE.names == ("candidate", "node_idx", "eligible", "n_victims", "num_violating",
                                            "first_priority", "sum_priorities", "earliest_start_unix_nano")
    assert abi.STRUCT_DTYPES[13] is abi.PREEMPT_PICK_DTYPE
    if os.path.exists(abi.LIB_PATH):
        assert abi.load_library().kg_abi_struct_size(13) == abi.PREEMPT_PICK_DTYPE.itemsize
