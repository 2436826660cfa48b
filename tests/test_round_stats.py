"""The control words the parity tests do not see: kg_stats of the schedule calls of tests/round_stats_cases.py equals
what tests/golden/round_stats.json recorded from the library of the commit before the control blocks got names and the
resolvers one shared bookkeeping (tests/golden/make_round_stats.py).  A swapped diagnostic word (pods re-scored on
the chain / the reserved word, rounds run / pods consumed) changes these numbers and no placement."""
import functools
import json
import os

import pytest

import round_stats_cases as C

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "round_stats.json")


@functools.lru_cache(maxsize=None)
def _want():
    with open(FIXTURE) as f:
        return json.load(f)["cases"]


@functools.lru_cache(maxsize=None)
def _got():
    return C.record()


def test_fixture_is_not_vacuous():
    """On the fixture alone: every case is there, some case re-scored pods on the chain and some case stopped a round
    early (more rounds than the pods need at full rounds)."""
    want = _want()
    assert set(want) == set(C.CASES)
    assert any(w.get("reserved0", 0) > 0 for w in want.values())
    assert any(want[name].get("device_batches", 0) > -(-pods // per) for name, (_, pods, per) in C.CASES.items())


@pytest.mark.parametrize("case", sorted(C.CASES))
def test_stats_equal_the_recorded(case):
    want, got = _want()[case], _got()[case]
    print(case, got)
    for field, value in want.items():
        if field == "active":  # a time: only that it was counted where it was counted before
            assert got[field] or not value, (case, field)
        else:
            assert got[field] == value, (case, field, got[field], value)
