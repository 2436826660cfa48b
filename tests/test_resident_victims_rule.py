"""tests/victims_reference.py against hand-derived cases, one per clause of the rule (no device)."""
from victims_reference import can_preempt, more_important_order, node_victims


def _nv(prio, start=None, quota=None, nonpre=None, mask=None, pdb=(), pod_priority=100, pod_quota=1, quota_rule=True):
    n = len(prio)
    return node_victims(pod_priority, pod_quota, quota_rule, prio, start or [0] * n, quota or [1] * n,
                        nonpre or [0] * n, mask or [0] * n, pdb)


def test_equal_priority_is_not_a_victim():
    assert _nv([100, 99, 101]).order == [1]
    assert _nv([100, 99, 101], quota_rule=False).order == [1]


def test_non_preemptible_is_kept_only_under_the_quota_rule():
    assert _nv([0, 0], nonpre=[1, 0]).order == [1]
    assert _nv([0, 0], nonpre=[1, 0], quota_rule=False).order == [0, 1]
    assert not can_preempt(100, 1, 0, 1, True, True) and can_preempt(100, 1, 0, 1, True, False)


def test_quota_mismatch():
    assert _nv([0, 0, 0], quota=[1, 2, 0]).order == [0]
    assert _nv([0, 0, 0], quota=[1, 2, 0], quota_rule=False).order == [0, 1, 2]


def test_budget_of_one_with_three_matching_pods():
    """the first stays clean, the next two violate; the violating group leads"""
    v = _nv([0, 0, 0], mask=[1, 1, 1], pdb=[1])
    assert v.order == [1, 2, 0] and v.violating == [True, True, False] and v.reordered


def test_pod_in_two_pdbs_one_exhausted():
    """pod 0 uses up PDB 1; pod 1 matches PDB 0 (room for 5) and PDB 1 (exhausted): violating"""
    v = _nv([50, 40], mask=[0b10, 0b11], pdb=[5, 1])
    assert v.order == [1, 0] and v.violating == [True, False]


def test_budget_of_zero():
    v = _nv([0, 0], mask=[1, 0], pdb=[0])
    assert v.order == [0, 1] and v.violating == [True, False] and not v.reordered


def test_mask_zero_never_violates():
    v = _nv([0, 0], mask=[0, 0], pdb=[0, 0])
    assert v.order == [0, 1] and v.violating == [False, False]


def test_every_matching_pdb_is_decremented():
    """pod 0 (in PDBs 0 and 1) violates through PDB 0 and still uses up PDB 1, so pod 1 violates too"""
    v = _nv([50, 40], mask=[0b11, 0b10], pdb=[0, 1])
    assert v.violating == [True, True] and v.order == [0, 1]


def test_order_priority_then_start_ties_keep_the_callers_order():
    prio, start = [10, 50, 10, 50, 10], [7, 9, 3, 9, 7]
    assert more_important_order(range(5), prio, start) == [1, 3, 2, 0, 4]
    v = _nv(prio, start=start)
    assert v.stored == [1, 3, 2, 0, 4] and v.order == [1, 3, 2, 0, 4]


def test_violating_group_precedes_the_others_each_in_order():
    # sorted: 3 (90), 0 (80), 2 (70), 1 (60); budget 1 on PDB 0 held by 3, 2, 1: 3 clean, 2 and 1 violating
    v = _nv([80, 60, 70, 90], mask=[0, 1, 1, 1], pdb=[1])
    assert v.order == [2, 1, 3, 0] and v.violating == [True, True, False, False] and v.reordered


def test_the_budgets_are_fresh_per_node():
    a = _nv([0], mask=[1], pdb=[1])
    b = _nv([0], mask=[1], pdb=[1])
    assert a.violating == b.violating == [False]
