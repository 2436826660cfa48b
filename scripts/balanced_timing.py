#!/usr/bin/env python
"""Times NodeResourcesBalancedAllocation on the round engine at the C3 size: 100k nodes, the C3 queue
(synth.make_pods_stream) and the C3 geometry (batch_pods 38, 8 pods per wave, the default pipeline depth).  Three
variants:

  fit-la           Fit + LoadAware (the C3 profile) on this build
  fit-la-bal       Fit + LoadAware + BalancedAllocation (weights 1 / 1 / 1) on this build: the round engine
  fit-la-bal@parent  the same profile on the library of the parent commit (--parent-lib, loaded through KOORDGPU_LIB):
                   the batched exact rounds

Per variant and repetition a fresh process (one library per process) stages the queue on a fresh engine, schedules
--warmup pods untimed and then --pods pods in one kg_pods_schedule_staged call; the variants alternate.  Prints one JSON
line and, with --out, writes it to a file:

  pods_per_s           median over the repetitions (wall time of the timed call), and every sample
  rescored_per_pod     kg_stats.reserved[0] / pods (round engine: the share of pods whose resolver step re-scored the
                       modified rows)
  resolver_active_s    kg_stats.reserved[2] (round engine: the resolvers' time from the chain hand-off to the publish)
  head_over_parent     fit-la-bal / fit-la-bal@parent, and the parent's run-to-run spread (max / min of its samples)
  bal_over_fit_la      fit-la-bal / fit-la on this build

    python scripts/balanced_timing.py --parent-lib PATH [--nodes 100000] [--pods 30000] [--warmup 2000] [--reps 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = ("fit-la", "fit-la-bal", "fit-la-bal@parent")


def one(variant, nodes, n_pods, warmup):
    from koordinator_amd import abi
    abi.OPTIONAL_SYMBOLS = ("kg_debug_balanced",)  # the parent's library lacks the entry point added since
    import bench  # the C3 workload's geometry
    from koordinator_amd import Engine, framework as F, synth
    _, _, batch, ppw, _ = bench.WORKLOADS["c3"]
    FIT, LA, BAL = F.NODE_RESOURCES_FIT, F.LOAD_AWARE, F.BALANCED_ALLOCATION
    score = {FIT: 1, LA: 1} if variant == "fit-la" else {FIT: 1, LA: 1, BAL: 1}
    cfg = F.build_config(profile=F.Profile(filter=(FIT, LA), score=score), batch_pods=batch, pods_per_wave=ppw)
    cluster = synth.make_cluster(nodes)
    pods = synth.make_pods_stream(warmup + n_pods)
    with Engine(cfg, cluster.n) as e:
        synth.load_into(e, cluster)
        e.stage(pods)
        if warmup:
            e.schedule_staged(0, warmup)
        t0 = time.perf_counter()
        st = e.schedule_staged(warmup, n_pods)
        dt = time.perf_counter() - t0
        node, _ = e.fetch(warmup, n_pods)
    return {"pods_per_s": n_pods / dt, "seconds": dt, "rescored_per_pod": float(st["reserved"][0]) / n_pods,
            "resolver_active_s": float(st["reserved"][2]), "rounds": int(st["device_batches"]),
            "placed": int((node >= 0).sum()), "distinct_nodes": int(len(set(node[node >= 0].tolist()))),
            "placement_hash": int(sum((int(x) + 2) * (i % 1009 + 1) for i, x in enumerate(node.tolist())) % (1 << 61))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=100_000)
    ap.add_argument("--pods", type=int, default=30_000)
    ap.add_argument("--warmup", type=int, default=2_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="libkoordgpu.so built from the parent commit")
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        print(json.dumps(one(a.one, a.nodes, a.pods, a.warmup)))
        return
    variants = [v for v in VARIANTS if a.parent_lib or not v.endswith("@parent")]
    samples = {v: [] for v in variants}
    for _ in range(a.reps):
        for v in variants:
            env = dict(os.environ)
            if v.endswith("@parent"):
                env["KOORDGPU_LIB"] = os.path.abspath(a.parent_lib)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", v, "--nodes", str(a.nodes), "--pods",
                                str(a.pods), "--warmup", str(a.warmup)], env=env, capture_output=True, text=True,
                               timeout=600)
            if r.returncode != 0:
                sys.exit(f"{v}: exit {r.returncode}\n{r.stderr[-2000:]}")
            samples[v].append(json.loads(r.stdout.strip().splitlines()[-1]))
    out = {"nodes": a.nodes, "pods": a.pods, "warmup": a.warmup, "reps": a.reps}
    for v in variants:
        s = samples[v]
        out[v] = {"pods_per_s": round(statistics.median(x["pods_per_s"] for x in s), 1),
                  "samples_pods_per_s": [round(x["pods_per_s"], 1) for x in s],
                  "seconds": round(statistics.median(x["seconds"] for x in s), 6),
                  "rescored_per_pod": round(s[0]["rescored_per_pod"], 4),
                  "resolver_active_s": round(statistics.median(x["resolver_active_s"] for x in s), 6),
                  "rounds": s[0]["rounds"], "placed": s[0]["placed"], "distinct_nodes": s[0]["distinct_nodes"],
                  "placement_hash": s[0]["placement_hash"]}
    out["bal_over_fit_la"] = round(out["fit-la-bal"]["pods_per_s"] / out["fit-la"]["pods_per_s"], 4)
    if a.parent_lib:
        p = out["fit-la-bal@parent"]
        out["head_over_parent"] = round(out["fit-la-bal"]["pods_per_s"] / p["pods_per_s"], 3)
        out["parent_spread"] = round(max(p["samples_pods_per_s"]) / min(p["samples_pods_per_s"]), 4)
        out["same_placements"] = out["fit-la-bal"]["placement_hash"] == p["placement_hash"]
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
