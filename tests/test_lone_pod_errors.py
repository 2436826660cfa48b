"""Error parity of the single-pod entry points across the LonePod refactor: every (profile, entry point, bad pod) of
tests/lone_pod_cases.py answers with the return code and the kg_last_error() text recorded in
tests/golden/lone_pod_errors.json from the library of the commit before the refactor
(tests/golden/make_lone_pod_errors.py).  A pair the earlier library accepted was recorded as code 0 and must stay 0.
The pods that are wrong in two ways pin which error wins."""
import functools
import json
import os

import pytest

import lone_pod_cases as L

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lone_pod_errors.json")
ENTRIES = ("evaluate_reservation", "debug_topn", "diagnose@0", "diagnose@3", "filter_preemption", "select_victims",
           "preempt", "evaluate_numa", "evaluate_device")


@functools.lru_cache(maxsize=None)
def _want():
    with open(FIXTURE) as f:
        return json.load(f)["answers"]


@functools.lru_cache(maxsize=None)
def _got():
    return L.record()


def test_fixture_covers_the_list():
    """On the fixture alone: every profile, entry point and case is there; each listed fault is refused somewhere, each
    entry point refuses something and accepts something, and the two-fault pods are refused with different texts by
    different entry points or profiles (so precedence is pinned, not vacuous)."""
    want = _want()
    assert set(want) == set(L.PROFILES)
    for per in want.values():
        assert set(per) == set(ENTRIES)
        for cases in per.values():
            assert set(cases) == set(L.CASES)
    for case in L.CASES:
        assert any(want[p][e][case][0] != 0 for p in want for e in ENTRIES), case
    for e in ENTRIES:
        codes = [want[p][e][c][0] for p in want for c in L.CASES]
        assert any(codes) and not all(codes), e
    for case in ("reserve_pod+bad_qos", "bad_qos+negative_device"):
        texts = {want[p][e][case][1] for p in want for e in ENTRIES if want[p][e][case][0] != 0}
        assert len(texts) >= 2, (case, texts)


@pytest.mark.parametrize("profile", sorted(L.PROFILES))
def test_codes_and_texts_equal_the_recorded(profile):
    want, got = _want()[profile], _got()[profile]
    for entry in ENTRIES:
        for case in L.CASES:
            assert got[entry][case] == want[entry][case], (profile, entry, case)
