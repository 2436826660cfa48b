#!/usr/bin/env python
"""Times the FitError counts of large (24-core and up) pods two ways, in one process, and prints one JSON line:

  device  Engine.diagnose(pods) for batches of 1, 16 and 256 pods: every Filter on every node and the per-reason /
          per-plugin counts on the GPU, one copy of sizeof(kg_fit_diag) bytes per pod back
  host    what a caller had to do before kg_pods_diagnose, per pod: Engine.evaluate (plus evaluate_numa /
          evaluate_device / evaluate_reservation on the shipped profile: one n-row vector per plugin across PCIe), then
          the first-failing-plugin composition and the counting in numpy

at the C3 size (Fit + LoadAware, 100k nodes) and at the shipped profile's size (Fit + LoadAware + NodeNUMAResource +
DeviceShare + Reservation, 50k nodes).  Median of --calls calls each after --warmup calls; ms per call, us per pod and
device-to-host bytes per pod.  The host path's shipped composition takes NodeNUMAResource from the plugin-alone evaluate
call (the un-restored NodeInfo), which is all that call offers; the host path is timed, not checked, here.

    python scripts/diag_timing.py [--calls 200] [--warmup 20] [--c3-nodes 100000] [--shipped-nodes 50000]
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

BATCHES = (1, 16, 256)
FIT_BITS = abi.REJECT_FIT_PODS | abi.REJECT_FIT_CPU | abi.REJECT_FIT_MEMORY | abi.REJECT_FIT_OTHER
BITS = (0, 1, 2, 3, 5, 6, 7, 8, 12, 13)


def _count(words):
    valid = words != abi.REJECT_INVALID_NODE
    out = {"num_all_nodes": int(valid.sum()), "feasible": int((words == 0).sum())}
    out["reasons"] = [int((valid & ((words >> b) & 1 != 0)).sum()) for b in BITS]
    out["fit_nodes"] = int((valid & ((words & FIT_BITS) != 0)).sum())
    return out


def host_wide(e, pod):
    rej, fit, la = e.evaluate(pod)
    words = np.where(rej & FIT_BITS, rej & FIT_BITS, rej)  # LoadAware's bit only where NodeResourcesFit passes
    return _count(words), rej.nbytes + fit.nbytes + la.nbytes


def host_shipped(e, pod):
    rej, _, _ = e.evaluate(pod)
    nok, _, _ = e.evaluate_numa(pod)
    dok, _ = e.evaluate_device(pod)
    ev = e.evaluate_reservation(pod)
    words = np.where(rej & FIT_BITS, rej & FIT_BITS, rej)
    words = np.where((words == 0) & (nok == 0), abi.REJECT_NUMA, words)
    words = np.where((words == 0) & (dok == 0), abi.REJECT_DEVICE, words)
    words = np.where((words == 0) & (ev["pass"] == 0), abi.REJECT_RESERVATION, words)
    n = len(rej)
    return _count(words), 8 * abi.RSV_EVAL_WORDS * n + 20 * n + 20 * n + 12 * n


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
        pods = synth.make_pods(max(BATCHES), seed=synth.BASE_SEED + 7)
        load = lambda e: synth.load_into(e, cluster)  # noqa: E731
        host = host_wide
    else:
        cluster, numa, dev, rsv = synth.make_shipped_cluster(n)
        pods = synth.make_shipped_pods(max(BATCHES), seed=synth.BASE_SEED + 7)
        pods["quota_id"] = 0
        load = lambda e: synth.load_shipped_into(e, cluster, numa, dev, rsv)  # noqa: E731
        host = host_shipped
    # large pods (at least 24 cores), so that a share of the nodes answers with a reason; the device's work does not
    # depend on that share (every Filter runs on every node), feasible_share reports it
    pods["requests"][:, abi.RES_CPU] = np.maximum(pods["requests"][:, abi.RES_CPU], 24_000)
    pods["nonzero_requests"][:, 0] = pods["requests"][:, abi.RES_CPU]
    out = {"nodes": n, "device": {}}
    with Engine(cfg, n) as e:
        load(e)
        d = e.diagnose(pods)
        out["feasible_share"] = round(float((d["feasible"] / np.maximum(d["num_all_nodes"], 1)).mean()), 4)
        for b in BATCHES:
            ms = median_ms(lambda: e.diagnose(pods[:b]), calls, warmup)
            out["device"][str(b)] = {"ms_per_call": round(ms, 4), "us_per_pod": round(1e3 * ms / b, 2),
                                     "bytes_per_pod": abi.FIT_DIAG_DTYPE.itemsize}
        ms = median_ms(lambda: e.diagnose(pods[:16], node_status=True), max(calls // 4, 1), max(warmup // 4, 1))
        out["device_with_status_16"] = {"ms_per_call": round(ms, 4), "us_per_pod": round(1e3 * ms / 16, 2),
                                        "bytes_per_pod": abi.FIT_DIAG_DTYPE.itemsize + 4 * n}
        _, host_bytes = host(e, pods[0])
        ms = median_ms(lambda: host(e, pods[0]), calls, warmup)
        out["host"] = {"ms_per_call": round(ms, 4), "us_per_pod": round(1e3 * ms, 2), "bytes_per_pod": int(host_bytes)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--c3-nodes", type=int, default=100_000)
    ap.add_argument("--shipped-nodes", type=int, default=50_000)
    a = ap.parse_args()
    out = {"calls": a.calls, "c3": run("c3", a.c3_nodes, a.calls, a.warmup),
           "shipped": run("shipped", a.shipped_nodes, a.calls, a.warmup)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
