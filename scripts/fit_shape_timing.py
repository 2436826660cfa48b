#!/usr/bin/env python
"""Times the round engine under NodeResourcesFit RequestedToCapacityRatio — the rising shape [(0,0),(100,10)] and the
falling shape [(0,10),(100,0)] — against MostAllocated and LeastAllocated on the same build, at the C3 size: 100k nodes,
the C3 queue (synth.make_pods_stream) and the C3 geometry (batch_pods 38, 8 pods per wave, the default pipeline depth),
Fit + LoadAware.  Per variant and repetition a fresh engine stages the queue, schedules --warmup pods untimed and then
--pods pods in one kg_pods_schedule_staged call; the variants alternate.  Prints one JSON line and, with --out, writes it
to a file:

  pods_per_s           median over the repetitions (wall time of the timed call), and every sample
  rescored_per_pod     kg_stats.reserved[0] / pods: the share of pods whose resolver step re-scored the modified rows
  rounds               device rounds of the timed call
  seconds              median wall time of the timed call; resolver_active_s: kg_stats.reserved[2], the resolvers' time
                       from the chain hand-off to the publish summed over the call's rounds (medians)
  ratio_to_most        the variant's pods/s over MostAllocated's (the yardstick: the same resolver rule, the parent's
                       kernels); ratio_to_least likewise

    python scripts/fit_shape_timing.py [--nodes 100000] [--pods 30000] [--warmup 2000] [--reps 3] [--out FILE]
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

RTCR = F.REQUESTED_TO_CAPACITY_RATIO
VARIANTS = {
    "LeastAllocated": F.NodeResourcesFitArgs(scoring_strategy="LeastAllocated"),
    "MostAllocated": F.NodeResourcesFitArgs(scoring_strategy="MostAllocated"),
    "RTCR-rising": F.NodeResourcesFitArgs(scoring_strategy=RTCR, shape=[(0, 0), (100, 10)]),
    "RTCR-falling": F.NodeResourcesFitArgs(scoring_strategy=RTCR, shape=[(0, 10), (100, 0)]),
}


def one(cluster, pods, fit, batch, ppw, warmup):
    cfg = F.build_config(fit=fit, batch_pods=batch, pods_per_wave=ppw)
    with Engine(cfg, cluster.n, fit_shape=fit.shape) as e:
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
            "seconds": dt, "resolver_active_s": float(st["reserved"][2]),
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
    samples = {v: [] for v in VARIANTS}
    for _ in range(a.reps):
        for v, fit in VARIANTS.items():
            samples[v].append(one(cluster, pods, fit, batch, ppw, a.warmup))
    out = {"nodes": a.nodes, "pods": a.pods, "warmup": a.warmup, "batch_pods": batch, "pods_per_wave": ppw, "reps": a.reps}
    for v in VARIANTS:
        out[v] = {"pods_per_s": round(statistics.median(x["pods_per_s"] for x in samples[v]), 1),
                  "samples_pods_per_s": [round(x["pods_per_s"], 1) for x in samples[v]],
                  "rescored_per_pod": round(samples[v][0]["rescored_per_pod"], 4), "rounds": samples[v][0]["rounds"],
                  "seconds": round(statistics.median(x["seconds"] for x in samples[v]), 6),
                  "resolver_active_s": round(statistics.median(x["resolver_active_s"] for x in samples[v]), 6),
                  "placed": samples[v][0]["placed"], "distinct_nodes": samples[v][0]["distinct_nodes"]}
    for v in ("RTCR-rising", "RTCR-falling"):
        out[v]["ratio_to_most"] = round(out[v]["pods_per_s"] / out["MostAllocated"]["pods_per_s"], 4)
        out[v]["ratio_to_least"] = round(out[v]["pods_per_s"] / out["LeastAllocated"]["pods_per_s"], 4)
    out["most_to_least"] = round(out["MostAllocated"]["pods_per_s"] / out["LeastAllocated"]["pods_per_s"], 4)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
