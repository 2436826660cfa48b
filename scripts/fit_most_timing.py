#!/usr/bin/env python
"""Times the round engine under NodeResourcesFit MostAllocated against LeastAllocated on the same build, at the C3 size:
100k nodes, the C3 queue (synth.make_pods_stream) and the C3 geometry (batch_pods 38, 8 pods per wave, the default
pipeline depth), Fit + LoadAware.  Per strategy and repetition a fresh engine stages the queue, schedules --warmup pods
untimed and then --pods pods in one kg_pods_schedule_staged call; the two strategies alternate.  Prints one JSON line
and, with --out, writes it to a file:

  pods_per_s           median over the repetitions (wall time of the timed call), and every sample
  rescored_per_pod     kg_stats.reserved[0] / pods: the share of pods whose resolver step re-scored the modified rows
  rounds               device rounds of the timed call
  ratio                MostAllocated pods/s over LeastAllocated pods/s

    python scripts/fit_most_timing.py [--nodes 100000] [--pods 30000] [--warmup 2000] [--reps 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (the C3 workload's geometry)
from koordinator_amd import Engine, framework as F, synth  # noqa: E402

STRATEGIES = ("LeastAllocated", "MostAllocated")


def one(cluster, pods, strategy, batch, ppw, warmup):
    cfg = F.build_config(fit=F.NodeResourcesFitArgs(scoring_strategy=strategy), batch_pods=batch, pods_per_wave=ppw)
    with Engine(cfg, cluster.n) as e:
        synth.load_into(e, cluster)
        e.stage(pods)
        if warmup:
            e.schedule_staged(0, warmup)
        t0 = time.perf_counter()
        st = e.schedule_staged(warmup, len(pods) - warmup)
        dt = time.perf_counter() - t0
        node, _ = e.fetch(warmup, len(pods) - warmup)
    n = len(pods) - warmup
    return {"pods_per_s": n / dt, "rescored_per_pod": float(st["reserved"][0]) / n, "rounds": int(st["device_batches"]),
            "placed": int((node >= 0).sum()), "distinct_nodes": int(len(set(node[node >= 0].tolist())))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=bench.WORKLOADS["c3"][0])
    ap.add_argument("--pods", type=int, default=30_000)
    ap.add_argument("--warmup", type=int, default=2_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _, _, batch, ppw, _ = bench.WORKLOADS["c3"]
    cluster = synth.make_cluster(a.nodes)
    pods = synth.make_pods_stream(a.warmup + a.pods)
    samples = {s: [] for s in STRATEGIES}
    for _ in range(a.reps):
        for s in STRATEGIES:
            samples[s].append(one(cluster, pods, s, batch, ppw, a.warmup))
    out = {"nodes": a.nodes, "pods": a.pods, "warmup": a.warmup, "batch_pods": batch, "pods_per_wave": ppw, "reps": a.reps}
    for s in STRATEGIES:
        out[s] = {"pods_per_s": round(statistics.median(x["pods_per_s"] for x in samples[s]), 1),
                  "samples_pods_per_s": [round(x["pods_per_s"], 1) for x in samples[s]],
                  "rescored_per_pod": round(samples[s][0]["rescored_per_pod"], 4), "rounds": samples[s][0]["rounds"],
                  "placed": samples[s][0]["placed"], "distinct_nodes": samples[s][0]["distinct_nodes"]}
    out["ratio"] = round(out["MostAllocated"]["pods_per_s"] / out["LeastAllocated"]["pods_per_s"], 4)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
