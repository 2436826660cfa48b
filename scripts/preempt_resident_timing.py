#!/usr/bin/env python
"""Times PostFilter over the resident bound-pod table against the call it replaces, and writes one JSON line (stdout
and --out):

  resident   kg_pods_preempt_resident: one pod record and a PDB budget vector up, the pick and the winner's victims back;
  parent     kg_pods_preempt over explicit victim lists, from a library built from the PARENT commit (--parent-lib),
             never the new code.  Each parent measurement is a child process of this script with KOORDGPU_LIB set to
             that library (two builds of one library cannot share a process: their exported symbols would bind to
             whichever was loaded first), started three times, interleaved with the resident measurements of this
             process; the spread of the baseline is the range of the three medians;
  set        kg_node_bound_pods_set for the whole table once, and for one node's list (median of --calls).

on the 100k-node Fit + LoadAware cluster of scripts/preempt_timing.py (about 600k bound pods), with every node a
candidate and over the nodes that fail or need victims.  Both sides see the same pods, priorities and start times and
the upstream rule (lower priority only, no PDBs), and the explicit lists are given in MoreImportantPod order with the
preemptor's priority above every pod's, so both pick among the same victims; the picks are compared before timing.
C entry points on arrays flattened once (what a Go caller pays), host wall clock per call, median of --calls after
--warmup.

    python scripts/preempt_resident_timing.py --parent-lib ab/libkoordgpu_parent.so [--nodes 100000] [--calls 200]
                                              [--warmup 20] [--out profiles/preempt_resident_timing.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from koordinator_amd import Engine, abi, framework as F, synth  # noqa: E402
from koordinator_amd.abi import check, ptr  # noqa: E402

PRIOS = np.array([0, 100, 1000], dtype=np.int32)
POD_PRIORITY = 2000  # above every bound pod's: the explicit lists hold every pod of the node, as the parent's timing did


def median_ms(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(t), 4)


def workload(n):
    """the cluster and its bound pods grouped by node, each node's list in MoreImportantPod order"""
    cluster = synth.make_cluster(n)
    rng = np.random.default_rng(synth.BASE_SEED + 9)
    prio = rng.choice(PRIOS, len(cluster.existing_pods))
    start = (16 * 10**17 + rng.integers(0, 10**6, len(prio)) * 10**9).astype(np.int64)
    order = np.lexsort((start, -prio.astype(np.int64), cluster.existing_node))
    bounds = np.searchsorted(cluster.existing_node[order], np.arange(n + 1)).astype(np.int64)
    vic = np.ascontiguousarray(cluster.existing_pods[order])
    vic["uid"] = 1 + np.arange(len(vic))
    return cluster, vic, np.ascontiguousarray(prio[order]), np.ascontiguousarray(start[order]), bounds


def explicit_arrays(nodes, vic, prio, start, bounds):
    counts = bounds[nodes + 1] - bounds[nodes]
    off = np.zeros(len(nodes) + 1, dtype=np.int64)
    off[1:] = np.cumsum(counts)
    take = (np.concatenate([np.arange(bounds[i], bounds[i + 1]) for i in nodes]) if off[-1]
            else np.zeros(0, dtype=np.int64))
    return off, np.ascontiguousarray(vic[take]), np.ascontiguousarray(prio[take]), np.ascontiguousarray(start[take])


def explicit_call(e, pod, nodes, off, vic, prio, start):
    """kg_pods_preempt over explicit lists → (call, pick, positions, status words)"""
    pick = np.zeros(1, dtype=abi.PREEMPT_PICK_DTYPE)
    cap = int(np.diff(off).max(initial=0))
    pv = np.zeros(max(cap, 1), dtype=np.int32)
    rej = np.zeros(len(nodes), dtype=np.int32)

    def call(want_rej=None):
        check(e.lib, e.lib.kg_pods_preempt(e.h, ptr(pod), len(nodes), ptr(nodes), ptr(off), ptr(vic), None, None, None,
                                           ptr(prio), ptr(start), ptr(pick), ptr(pv), cap, ptr(want_rej)))
    return call, pick, pv, rej


def needing_nodes(e, pod, n, vic, prio, start, bounds):
    """the nodes that fail or need victims, from the existing kg_pods_select_victims over every node"""
    nodes = np.arange(n, dtype=np.int32)
    off, v, _, _ = explicit_arrays(nodes, vic, prio, start, bounds)
    rej, kept, nvio = np.zeros(n, np.int32), np.zeros(max(int(off[-1]), 1), np.uint8), np.zeros(n, np.int32)
    check(e.lib, e.lib.kg_pods_select_victims(e.h, ptr(pod), n, ptr(nodes), ptr(off), ptr(v), None, None, None, ptr(rej),
                                              ptr(kept), ptr(nvio)))
    any_kept = np.add.reduceat(np.append(kept[:int(off[-1])], 0), np.minimum(off[:-1], int(off[-1]))) * (np.diff(off) > 0) > 0
    return nodes[(rej != 0) | any_kept]


def parent_role(a):
    """child process: kg_pods_preempt of the library KOORDGPU_LIB names, both shapes → one JSON line"""
    # the parent's library predates the resident entry points
    abi.OPTIONAL_SYMBOLS = ("kg_node_bound_pods_set", "kg_nodes_read_bound_pods", "kg_pods_select_victims_resident",
                            "kg_pods_preempt_resident")
    n = a.nodes
    cluster, vic, prio, start, bounds = workload(n)
    pod = F.make_pod(requests={"cpu": "24", "memory": "48Gi"})
    out = {}
    with Engine(F.build_config(), n) as e:
        synth.load_into(e, cluster)
        needs = needing_nodes(e, pod, n, vic, prio, start, bounds)
        for name, nodes in (("every_node", np.arange(n, dtype=np.int32)), ("nodes_needing_preemption", needs)):
            call, pick, pv, _ = explicit_call(e, pod, nodes, *explicit_arrays(nodes, vic, prio, start, bounds))
            out[name] = {"ms": median_ms(call, a.calls, a.warmup), "candidates": len(nodes),
                         "pick": [int(pick[0][k]) for k in abi.PREEMPT_PICK_DTYPE.names]}
    print("PARENT " + json.dumps(out))


def run_parent(a):
    env = dict(os.environ, KOORDGPU_LIB=os.path.abspath(a.parent_lib))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--role", "parent", "--nodes", str(a.nodes), "--calls",
                        str(a.calls), "--warmup", str(a.warmup)], env=env, check=True, capture_output=True, text=True,
                       timeout=900)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("PARENT ")][-1]
    return json.loads(line[len("PARENT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=100_000)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--parent-lib", default=None, help="libkoordgpu.so built from the parent commit")
    ap.add_argument("--role", default="main", choices=("main", "parent"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.role == "parent":
        return parent_role(a)
    n = a.nodes
    cluster, vic, prio, start, bounds = workload(n)
    pod = F.make_pod(requests={"cpu": "24", "memory": "48Gi"})
    out = {"nodes": n, "calls": a.calls, "bound_pods": int(len(vic)), "parent": [], "resident_ms": {}}
    shapes = ("every_node", "nodes_needing_preemption")
    with Engine(F.build_config(), n) as e:
        synth.load_into(e, cluster)
        all_nodes = np.arange(n, dtype=np.int32)
        needs = needing_nodes(e, pod, n, vic, prio, start, bounds)
        # the table: the whole cluster in one call, then one node's list again and again
        off_all = bounds.copy()
        t0 = time.perf_counter()
        check(e.lib, e.lib.kg_node_bound_pods_set(e.h, n, ptr(all_nodes), ptr(off_all), ptr(vic), ptr(prio), ptr(start),
                                                  None, None, None))
        out["set_whole_table_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        i = int(np.argmax(np.diff(bounds)))
        one = np.array([i], dtype=np.int32)
        o1 = np.array([0, bounds[i + 1] - bounds[i]], dtype=np.int64)
        sl = slice(bounds[i], bounds[i + 1])
        v1, p1, s1 = (np.ascontiguousarray(x[sl]) for x in (vic, prio, start))
        out["set_one_node_ms"] = {"entries": int(o1[1]), "ms": median_ms(lambda: check(e.lib, e.lib.kg_node_bound_pods_set(
            e.h, 1, ptr(one), ptr(o1), ptr(v1), ptr(p1), ptr(s1), None, None, None)), a.calls, a.warmup)}
        pick = np.zeros(1, dtype=abi.PREEMPT_PICK_DTYPE)
        cap = int(np.diff(bounds).max())
        uid, idx = np.zeros(cap, np.int64), np.zeros(cap, np.int32)
        calls = {}
        for name, nodes in zip(shapes, (None, needs)):
            nc = n if nodes is None else len(nodes)
            rej = np.zeros(nc, dtype=np.int32)

            def call(want_rej=None, nodes=nodes, nc=nc):
                check(e.lib, e.lib.kg_pods_preempt_resident(e.h, ptr(pod), POD_PRIORITY, 0, nc, ptr(nodes), None, 0, ptr(pick),
                                                            ptr(uid), ptr(idx), cap, ptr(want_rej)))
            # the same answer as this library's kg_pods_preempt over the explicit lists
            cand = all_nodes if nodes is None else nodes
            x_off, x_vic, x_prio, x_start = explicit_arrays(cand, vic, prio, start, bounds)
            x_call, x_pick, x_pv, x_rej = explicit_call(e, pod, cand, x_off, x_vic, x_prio, x_start)
            x_call(x_rej)
            call(rej)
            assert pick[0].tolist() == x_pick[0].tolist() and np.array_equal(rej, x_rej), (name, pick, x_pick)
            nv = int(pick[0]["n_victims"])
            assert uid[:nv].tolist() == x_vic["uid"][x_pv[:nv]].tolist(), name
            calls[name] = call
            out["resident_ms"][name] = {"candidates": nc, "medians": [],
                                        "pick": [int(pick[0][k]) for k in abi.PREEMPT_PICK_DTYPE.names]}
        for _ in range(3):  # interleaved: parent child, then the resident call of this process
            if a.parent_lib:
                out["parent"].append(run_parent(a))
            for name in shapes:
                out["resident_ms"][name]["medians"].append(median_ms(calls[name], a.calls, a.warmup))
    out["verdict"] = {}
    for name in shapes:
        res = statistics.median(out["resident_ms"][name]["medians"])
        v = {"resident_ms": res}
        if out["parent"]:
            pm = [p[name]["ms"] for p in out["parent"]]
            assert all(p[name]["pick"] == out["resident_ms"][name]["pick"] for p in out["parent"]), name
            spread = max(pm) - min(pm)
            v.update(parent_medians_ms=pm, parent_spread_ms=round(spread, 4),
                     below_parent_by_more_than_its_spread=bool(res < min(pm) - spread))
        out["verdict"][name] = v
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
