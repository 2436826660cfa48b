#!/usr/bin/env python
"""Times the --debug-scores table of one pod two ways, in one process, and prints one JSON line:

  device  Engine.debug_topn(pod, 10): ranked and broken down on the GPU, one copy of 10 rows + two counters
  host    what a caller had to do before kg_debug_topn: the evaluate* calls (one n-row vector per plugin across
          PCIe), then NormalizeScore, the weights and the top-10 ranking in numpy

at the C3 size (Fit + LoadAware, 100k nodes) and at the shipped profile's size (Fit + LoadAware + NodeNUMAResource +
DeviceShare + Reservation, 50k nodes).  Median of --calls calls each after --warmup calls; bytes = device-to-host
bytes per call.  The host path's shipped composition takes Fit / LoadAware / NodeNUMAResource from the plugin-alone
evaluate calls (the un-restored NodeInfo), which is all those calls offer; it is timed, not checked, here.

    python scripts/topn_timing.py [--calls 200] [--warmup 20] [--c3-nodes 100000] [--shipped-nodes 50000]
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

import bench  # noqa: E402  (the workloads' profiles)
from koordinator_amd import Engine, abi, framework as F, synth  # noqa: E402

TOPN = 10


def _top(total, feasible, k):
    idx = np.flatnonzero(feasible)
    if len(idx) > k:  # the k best by (total desc, index asc): a partition on the packed key, then a sort of k
        key = (total[idx].astype(np.int64) << 32) | (0xFFFFFFFF - idx)
        idx = idx[np.argpartition(-key, k - 1)[:k]]
    return idx[np.lexsort((idx, -total[idx]))]


def host_wide(e, cfg, pod):
    rej, fit, la = e.evaluate(pod)
    total = int(cfg["weight_fit"]) * fit + int(cfg["weight_loadaware"]) * la
    return _top(total, rej == 0, TOPN), rej.nbytes + fit.nbytes + la.nbytes


def host_shipped(e, cfg, pod):
    ev = e.evaluate_reservation(pod)
    _, fit, la = e.evaluate(pod)
    _, nsc, naff = e.evaluate_numa(pod)
    _, dsc = e.evaluate_device(pod)
    feas = ev["pass"] == 1
    order = np.where(feas & (ev["order"] > 0), ev["order"], np.iinfo(np.int64).max)
    raw = np.where(feas, ev["score"], 0)
    if (order != np.iinfo(np.int64).max).any():
        raw[int(np.argmin(order))] = 1000
    mx = int(raw.max()) if feas.any() else 0
    mds = int(ev["ds_raw"][feas].max()) if feas.any() else 0
    total = ev["base"].copy()
    if mx > 0:
        total += int(cfg["weight_reservation"]) * (100 * raw // mx)
    if mds > 0:
        total += int(cfg["weight_deviceshare"]) * (100 * ev["ds_raw"] // mds)
    cols = (int(cfg["weight_fit"]) * fit, int(cfg["weight_loadaware"]) * la, int(cfg["weight_numa"]) * nsc)
    top = _top(total, feas, TOPN)
    _ = [c[top] for c in cols]
    nbytes = 8 * abi.RSV_EVAL_WORDS * len(feas) + 20 * len(feas) + 20 * len(feas) + 12 * len(feas)
    return top, nbytes


def median_ms(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t)


def run(name, n, calls, warmup):
    profile, la = bench.workload_profile(name)
    cfg = F.build_config(profile=profile, la=la)
    if name == "c3":
        cluster = synth.make_cluster(n)
        pod = synth.make_pods(8)[3]
        load = lambda e: synth.load_into(e, cluster)  # noqa: E731
        host = host_wide
    else:
        cluster, numa, dev, rsv = synth.make_shipped_cluster(n)
        pod = synth.make_shipped_pods(8)[3]
        pod["quota_id"] = 0
        load = lambda e: synth.load_shipped_into(e, cluster, numa, dev, rsv)  # noqa: E731
        host = host_shipped
    with Engine(cfg, n) as e:
        load(e)
        rows, feasible = e.debug_topn(pod, TOPN)
        top, host_bytes = host(e, cfg[0], pod)
        dev_ms = median_ms(lambda: e.debug_topn(pod, TOPN), calls, warmup)
        host_ms = median_ms(lambda: host(e, cfg[0], pod), calls, warmup)
    return {"nodes": n, "feasible": feasible, "rows": len(rows), "device_ms": round(dev_ms, 4),
            "host_ms": round(host_ms, 4), "device_bytes": 16 + TOPN * abi.TOPN_ROW_DTYPE.itemsize,
            "host_bytes": int(host_bytes), "same_best_node": bool(len(top) and len(rows) and top[0] == rows["node_idx"][0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--c3-nodes", type=int, default=100_000)
    ap.add_argument("--shipped-nodes", type=int, default=50_000)
    a = ap.parse_args()
    out = {"topn": TOPN, "calls": a.calls, "c3": run("c3", a.c3_nodes, a.calls, a.warmup),
           "shipped": run("shipped", a.shipped_nodes, a.calls, a.warmup)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
