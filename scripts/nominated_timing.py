#!/usr/bin/env python
"""Times scheduling with a nominated-pod table at C3 size and writes one JSON line (stdout and --out):

  all_affected   pods/s of a queue every pod of which lies at or below the table's highest priority (64 entries): the
                 whole queue takes the exact per-pod pass with the table;
  one_percent    pods/s of a queue with 1 % affected pods, spread evenly: the other runs keep the round engine;
  empty          pods/s of the same queue through kg_pods_schedule_staged_nominated with an empty table (the plain call);
  set_64 / set_4096   microseconds per kg_nominated_pods_set of 64 and of 4096 entries (median of --calls).

on the 100k-node Fit + LoadAware cluster of bench.py's C3 workload.  The entries sit on the first nodes and are none
of the queue's pods, so no entry dies and every repetition sees the same table.  Host wall clock around the C entry
point on a staged queue, median of --reps schedule calls, each on a freshly loaded engine state.

    python scripts/nominated_timing.py [--nodes 100000] [--pods 20000] [--affected-pods 2000] [--reps 3]
                                       [--calls 50] [--out profiles/nominated/timing.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from koordinator_amd import Engine, abi, framework as F, synth  # noqa: E402


def entries(cluster, n):
    """n small entries of priority 100 on the first n nodes (node k % nodes), uids outside the queue's"""
    pods = np.zeros(n, dtype=abi.POD_DTYPE)
    pods["requests"][:, abi.RES_CPU] = 500
    pods["requests"][:, abi.RES_MEMORY] = 1 << 30
    pods["nonzero_requests"][:, 0] = 500
    pods["nonzero_requests"][:, 1] = 1 << 30
    pods["uid"] = 10**9 + np.arange(n)
    return pods, (np.arange(n) % cluster.n).astype(np.int32), np.full(n, 100, np.int32)


def pods_per_s(cfg, cluster, pods, prios, table, reps):
    rates, counters = [], None
    for _ in range(reps):
        with Engine(cfg, cluster.n) as e:
            synth.load_into(e, cluster)
            if table is not None:
                e.set_nominated(*table)
            e.stage(pods)
            t0 = time.perf_counter()
            e.schedule_staged(0, len(pods), prios)
            rates.append(len(pods) / (time.perf_counter() - t0))
            counters = e.nominated_counters()
    return round(statistics.median(rates), 1), [round(r, 1) for r in rates], counters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=100000)
    ap.add_argument("--pods", type=int, default=20000)
    ap.add_argument("--affected-pods", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nominated", "timing.json"))
    a = ap.parse_args()
    cfg = F.build_config(device_id=0)
    cluster = synth.make_cluster(a.nodes, seed=synth.BASE_SEED)
    pods = synth.make_pods_stream(a.pods, seed=synth.BASE_SEED + 1)
    pods["uid"] = 1 + np.arange(len(pods))
    table = entries(cluster, 64)
    out = {"nodes": a.nodes, "entries": 64, "reps": a.reps}
    few = pods[:a.affected_pods]
    r, runs, c = pods_per_s(cfg, cluster, few, np.zeros(len(few), np.int32), table, a.reps)
    out["all_affected"] = {"pods": len(few), "pods_per_s": r, "runs": runs, "counters": c}
    prios = np.full(len(pods), 1000, np.int32)
    prios[::100] = 0
    r, runs, c = pods_per_s(cfg, cluster, pods, prios, table, a.reps)
    out["one_percent"] = {"pods": len(pods), "pods_per_s": r, "runs": runs, "counters": c}
    r, runs, c = pods_per_s(cfg, cluster, pods, prios, None, a.reps)
    out["empty"] = {"pods": len(pods), "pods_per_s": r, "runs": runs, "counters": c}
    with Engine(cfg, cluster.n) as e:
        synth.load_into(e, cluster)
        for n in (64, abi.MAX_NOMINATED):
            t = entries(cluster, n)
            e.set_nominated(*t)
            us = []
            for _ in range(a.calls):
                t0 = time.perf_counter()
                e.set_nominated(*t)
                us.append((time.perf_counter() - t0) * 1e6)
            out[f"set_{n}_us"] = round(statistics.median(us), 1)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
