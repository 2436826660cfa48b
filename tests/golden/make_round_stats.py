#!/usr/bin/env python3
"""Writes tests/golden/round_stats.json: the kg_stats of the schedule calls of tests/round_stats_cases.py.

The fixture pins the control words behind kg_stats (rounds run, pods re-scored on the chain, the reserved word) across a
change of the resolvers' bookkeeping, so it is recorded against the library built from the commit BEFORE that change,
on a machine with the GPU:

    git worktree add /tmp/before <commit> && make -C /tmp/before/koordinator_amd
    KOORDGPU_LIB=/tmp/before/koordinator_amd/libkoordgpu.so python tests/golden/make_round_stats.py

Every case runs twice; a field that differs between the two runs is printed and left out of that case.  The recorder
refuses a fixture that proves nothing: some case must have re-scored pods on the chain (reserved0 > 0) and some case
must have stopped a round early (more rounds than ceil(pods / pods per round)).
tests/test_round_stats.py replays the calls against the library in the tree and compares the recorded fields exactly."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import round_stats_cases as C  # noqa: E402
from koordinator_amd import abi  # noqa: E402


def main():
    a, b = C.record(), C.record()
    cases = {}
    for name in C.CASES:
        keep = {k: v for k, v in a[name].items() if b[name][k] == v}
        for k in sorted(set(a[name]) - set(keep)):
            print(f"dropped {name}.{k}: {a[name][k]} then {b[name][k]}")
        cases[name] = keep
        print(name, keep)
    if not any(c.get("reserved0", 0) > 0 for c in cases.values()):
        sys.exit("no case re-scored a pod on the chain (reserved0 is 0 everywhere): pick other seeds")
    if not any(c.get("device_batches", 0) > -(-pods // per) for (_, pods, per), c in zip(C.CASES.values(), cases.values())):
        sys.exit("no case stopped a round early (device_batches = ceil(pods / pods per round) everywhere): pick other seeds")
    out = {"library": os.path.basename(abi.LIB_PATH), "abi_version": abi.ABI_VERSION, "cases": cases}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "round_stats.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{path}: {sum(len(c) for c in cases.values())} fields in {len(cases)} cases")


if __name__ == "__main__":
    main()
