#!/usr/bin/env python
"""Times PostFilter's "dry run, then pick one candidate" three ways on one engine, in one process, and writes one JSON
line (stdout and --out):

  a  the path without kg_pods_preempt: kg_pods_select_victims, its copy-back (a status word and a violating count per
     candidate, a byte per potential victim) and upstream's pickOneNodeForPreemption as vectorised numpy on the host.
     Uses nothing kg_pods_preempt added, so it runs the same on a checkout without it;
  b  kg_pods_preempt: the same dry run, the pick reduced on the device, one kg_preempt_pick and the winner's victims back;
  c  kg_pods_select_victims alone, for the share the dry-run kernel and its copies take of either.

on a Fit + LoadAware cluster (synth.make_cluster) with every node a candidate and its pods as the potential victims —
and again over only the nodes that fail or need victims, the candidates PostFilter would pass: among all nodes the first
one that needs no preemption wins at once and the host pick stops there.  Two levels: `abi` calls the C entry points on
arrays flattened once (what a Go caller pays), `engine` goes through Engine.select_victims / Engine.preempt, whose
per-call flattening of one Python list per node takes seconds at 100k nodes (hence --engine-calls, few).  Median of
--calls calls after --warmup; b is skipped (null) when the library has no kg_pods_preempt.  Before
timing, a's pick is checked against b's.

    python scripts/preempt_timing.py [--nodes 100000] [--calls 200] [--warmup 20] [--engine-calls 5] [--out profiles/preempt_timing.json]
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
from koordinator_amd.abi import check, ptr  # noqa: E402

PRIOS = np.array([0, 100, 1000], dtype=np.int32)


def host_pick(off, rej, kept, nvio, prio, start):
    """pickOneNodeForPreemption over select_victims' outputs, vectorised: (candidate, its victims' positions)"""
    elig = np.nonzero(rej == 0)[0]
    if len(elig) == 0:
        return -1, np.zeros(0, dtype=np.int64)
    k = kept != 0
    cnt = np.concatenate(([0], np.cumsum(k)))
    count = cnt[off[1:]] - cnt[off[:-1]]
    c = elig[count[elig] == 0]
    if len(c):
        return int(c[0]), np.zeros(0, dtype=np.int64)
    c = elig
    v = nvio[c]
    c = c[v == v.min()]
    if len(c) > 1:
        first = np.searchsorted(cnt, cnt[off[:-1]][c] + 1) - 1  # position of each candidate's first kept entry
        p0 = prio[first]
        c = c[p0 == p0.min()]
    if len(c) > 1:
        cs = np.concatenate(([0], np.cumsum(np.where(k, prio.astype(np.int64) + 2**31, 0))))
        s = cs[off[1:]][c] - cs[off[:-1]][c]
        c = c[s == s.min()]
    if len(c) > 1:
        n = count[c]
        c = c[n == n.min()]
    if len(c) > 1:
        ear = np.empty(len(c), dtype=np.int64)
        for q, w in enumerate(c):  # the few that tie this far
            sl = slice(off[w], off[w + 1])
            kp, pp, ss = k[sl], prio[sl], start[sl]
            ear[q] = ss[kp & (pp == pp[kp].max())].min()
        c = c[ear == ear.max()]
    w = int(c[0])
    return w, off[w] + np.nonzero(k[off[w]:off[w + 1]])[0]


def median_ms(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(t), 4)


def measure(e, pod, node_ids, vic_all, prio_all, start_all, bounds, calls, warmup, engine_calls):
    """the three paths over the candidates `node_ids` (each node's pods = vic_all[bounds[i]:bounds[i + 1]])"""
    n = len(node_ids)
    nodes = np.ascontiguousarray(node_ids, dtype=np.int32)
    counts = bounds[nodes + 1] - bounds[nodes]
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum(counts)
    nv = int(off[-1])
    take = np.concatenate([np.arange(bounds[i], bounds[i + 1]) for i in nodes]) if nv else np.zeros(0, dtype=np.int64)
    vic = np.ascontiguousarray(vic_all[take])
    prio = np.ascontiguousarray(prio_all[take])
    start = np.ascontiguousarray(start_all[take])
    cap = int(counts.max())
    out = {"candidates": n, "potential_victims": nv}
    lib, h = e.lib, e.h
    fused = hasattr(e, "preempt")
    rej = np.zeros(n, dtype=np.int32)
    kept = np.zeros(max(nv, 1), dtype=np.uint8)
    nvio = np.zeros(n, dtype=np.int32)
    pick = np.zeros(1, dtype=abi.PREEMPT_PICK_DTYPE) if fused else None
    pv = np.zeros(max(cap, 1), dtype=np.int32)

    def abi_c():
        check(lib, lib.kg_pods_select_victims(h, ptr(pod), n, ptr(nodes), ptr(off), ptr(vic), None, None, None,
                                              ptr(rej), ptr(kept), ptr(nvio)))

    def abi_a():
        abi_c()
        return host_pick(off, rej, kept, nvio, prio, start)

    def abi_b():
        check(lib, lib.kg_pods_preempt(h, ptr(pod), n, ptr(nodes), ptr(off), ptr(vic), None, None, None, ptr(prio),
                                       ptr(start), ptr(pick), ptr(pv), cap, None))

    w, wv = abi_a()
    out["eligible"] = int((rej == 0).sum())
    out["winner_victims"] = len(wv)
    out["copy_back_bytes"] = {"a": int(rej.nbytes + nvio.nbytes + nv), "b": None}
    if fused:
        abi_b()
        assert int(pick[0]["candidate"]) == w and pv[:len(wv)].tolist() == wv.tolist(), (pick, w)
        out["copy_back_bytes"]["b"] = int(abi.PREEMPT_PICK_DTYPE.itemsize + 4 * cap)
    out["abi_ms"] = {"a_select_victims_host_pick": median_ms(abi_a, calls, warmup),
                     "b_preempt": median_ms(abi_b, calls, warmup) if fused else None,
                     "c_select_victims": median_ms(abi_c, calls, warmup),
                     "host_pick_alone": median_ms(lambda: host_pick(off, rej, kept, nvio, prio, start), calls, warmup)}
    if engine_calls > 0:
        vics = [vic[off[c]:off[c + 1]] for c in range(n)]
        prios = [prio[off[c]:off[c + 1]] for c in range(n)]
        starts = [start[off[c]:off[c + 1]] for c in range(n)]

        def engine_a():
            r, k, v = e.select_victims(pod, nodes, vics)
            return host_pick(off, r, np.concatenate(k), v, prio, start)

        assert engine_a()[0] == w
        if fused:
            assert int(e.preempt(pod, nodes, vics, prios, starts)[0]["candidate"]) == w
        out["engine_ms"] = {"calls": engine_calls,
                            "a_select_victims_host_pick": median_ms(engine_a, engine_calls, 1),
                            "b_preempt": median_ms(lambda: e.preempt(pod, nodes, vics, prios, starts), engine_calls, 1)
                            if fused else None,
                            "c_select_victims": median_ms(lambda: e.select_victims(pod, nodes, vics), engine_calls, 1)}
    needs = nodes[(rej != 0) | (np.add.reduceat(np.append(kept[:nv], 0), np.minimum(off[:-1], nv)) * (counts > 0) > 0)]
    return out, needs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=100_000)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--engine-calls", type=int, default=5, help="calls per path at the Engine level (seconds each at "
                    "100k nodes: the binding flattens one list per node); 0 skips that level")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.nodes
    cluster = synth.make_cluster(n)
    rng = np.random.default_rng(synth.BASE_SEED + 9)
    order = np.argsort(cluster.existing_node, kind="stable")
    bounds = np.searchsorted(cluster.existing_node[order], np.arange(n + 1)).astype(np.int64)
    vic = cluster.existing_pods[order]
    prio = rng.choice(PRIOS, len(vic))
    start = (16 * 10**17 + rng.integers(0, 10**6, len(vic)) * 10**9).astype(np.int64)
    pod = F.make_pod(requests={"cpu": "24", "memory": "48Gi"})
    out = {"nodes": n, "calls": a.calls}
    with Engine(F.build_config(), n) as e:
        synth.load_into(e, cluster)
        # every node a candidate; then the candidates PostFilter would pass: the nodes that fail or need victims (among all
        # nodes the first that needs no preemption wins at rule 0, and the host pick stops there)
        out["every_node"], needs = measure(e, pod, np.arange(n), vic, prio, start, bounds, a.calls, a.warmup, a.engine_calls)
        out["nodes_needing_preemption"], _ = measure(e, pod, needs, vic, prio, start, bounds, a.calls, a.warmup, 0)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
