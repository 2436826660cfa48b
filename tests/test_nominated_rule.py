"""CPU: hand-derived known answers (tests/nominated_cases.py) pin the plain model of nominated pods
(tests/nominated_reference.py), which the GPU tests compare the device against."""
import numpy as np
import pytest

import nominated_reference as R
from koordinator_amd import framework as F
from nominated_cases import CASES


def run_model(case):
    cfg = F.build_config(profile=case.profile)
    cluster = case.cluster()
    table = R.Table(*case.table_arrays())
    numa = R.make_numa(np.concatenate(case.numa)) if case.numa else None
    st = R.initial_states(cfg, cluster)
    pods, prios = case.queue_arrays()
    filt = []
    for j, i, _, _ in case.filters:
        rej, added = R.filter_nominated(cfg, cluster, st, pods[j:j + 1], prios[j], table, numa)
        filt.append((j, i, int(rej[i]), int(added[i])))
    node, score, _ = R.schedule(cfg, cluster, pods, prios, table, numa, st)
    return list(zip(node.tolist(), score.tolist())), [u for u, _, _ in table.stored()], filt


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name.replace(" ", "_"))
def test_model_gives_the_known_answer(case):
    got, live, filt = run_model(case)
    assert got == case.want
    assert live == case.live_after
    assert filt == case.filters
