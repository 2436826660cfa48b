#!/usr/bin/env python3
"""Writes tests/golden/lone_pod_errors.json: what every single-pod entry point answers to the bad pods of
tests/lone_pod_cases.py — (return code, kg_last_error() text) per profile, entry point and case.

The fixture pins behaviour across a change of the host-side decode, so it is recorded against the library built from
the commit BEFORE that change, on a machine with the GPU:

    git worktree add /tmp/before <commit> && make -C /tmp/before/koordinator_amd
    KOORDGPU_LIB=/tmp/before/koordinator_amd/libkoordgpu.so python tests/golden/make_lone_pod_errors.py

tests/test_lone_pod_errors.py replays the same calls against the library in the tree and compares exactly."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import lone_pod_cases  # noqa: E402
from koordinator_amd import abi  # noqa: E402


def main():
    out = {"library": os.path.basename(abi.LIB_PATH), "abi_version": abi.ABI_VERSION, "answers": lone_pod_cases.record()}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "lone_pod_errors.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    refused = sum(v[0] != 0 for per in out["answers"].values() for cases in per.values() for v in cases.values())
    total = sum(len(cases) for per in out["answers"].values() for cases in per.values())
    print(f"{path}: {total} answers, {refused} refusals")


if __name__ == "__main__":
    main()
