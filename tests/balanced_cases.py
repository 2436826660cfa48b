"""Inputs shared by tests/test_balanced_rule.py (no GPU) and tests/test_balanced_round_gpu.py — TEST INFRASTRUCTURE.

KNOWN: hand-derived answers of the NodeResourcesBalancedAllocation rule.
scenario_listed / scenario_unlisted: the two situations in which a resolver that kept the monotone rule of DESIGN.md
§3.3 answers differently from sequential scheduling once BalancedAllocation is in the key.  Both run
the `balanced_only` profile (Fit Filter, Balanced 1) on nodes of 10 cpu / 100 GiB, so a key is the Balanced score alone:
100 − 50·|cpu fraction − memory fraction|, truncated."""
from __future__ import annotations

import numpy as np

from fit_strategy_cases import (BATCHES, DEPTHS, GI, MI, SEEDS, SIZES, Scenario, aux_inputs, parity_cluster,  # noqa: F401
                                parity_queue, pod, quota_inputs)
from koordinator_amd import abi, framework, synth

F = framework
FIT, LA, BAL = F.NODE_RESOURCES_FIT, F.LOAD_AWARE, F.BALANCED_ALLOCATION

# (alloc, requested, pod, resources, want, why) — (cpu milli, memory bytes) pairs
KNOWN = [
    ((4000, 8 * GI), (1000, 2 * GI), (1000, 2 * GI), 3, 100, "0.5 and 0.5: std 0"),
    ((4000, 8 * GI), (0, 0), (3000, 2 * GI), 3, 75, "0.75 and 0.25: std 0.25, (1 - 0.25)*100 = 75 exactly"),
    ((4000, 8 * GI), (0, 0), (3000, 2 * GI), 1, 100, "one resource configured (cpu): std 0"),
    ((4000, 8 * GI), (0, 0), (3000, 2 * GI), 2, 100, "one resource configured (memory): std 0"),
    ((0, 8 * GI), (0, 0), (3000, 6 * GI), 3, 100, "cpu allocatable 0: the resource is dropped, one is left, std 0"),
    ((4000, 0), (0, 0), (3000, 6 * GI), 3, 100, "memory allocatable 0: dropped"),
    ((4000, 8 * GI), (3500, 0), (1500, 2 * GI), 3, 62, "cpu 5000/4000 capped at 1, memory 0.25: std 0.375 -> 62.5 -> 62"),
    ((4000, 8 * GI), (9000, 16 * GI), (1000, 2 * GI), 3, 100, "both over-committed: both capped at 1, std 0"),
    ((3, 7), (1, 0), (0, 2), 3, 97, "1/3 and 2/7: std 1/42 = 0.0238..; 97.619.. -> 97"),
]


def go_balanced(alloc, req, pod, resources=3) -> int:
    """balancedResourceScorer with Python floats (IEEE binary64, as Go's float64): an independent restatement"""
    f = [min(float(req[r] + pod[r]) / float(alloc[r]), 1.0) for r in range(2) if resources >> r & 1 and alloc[r] != 0]
    std = abs((f[0] - f[1]) / 2) if len(f) == 2 else 0.0
    return int((1 - std) * 100.0)


def near_integer(alloc, req, pod, ulps: int = 2):
    """→ 0 when (1 − std)·100 of the triple, in Python floats, is farther than `ulps` ulp from every integer; else −1 /
    +1 for a value just below / just above one, 2 for an integer hit exactly (with std != 0)"""
    import math
    if alloc[0] == 0 or alloc[1] == 0:
        return 0
    f = [min(float(req[r] + pod[r]) / float(alloc[r]), 1.0) for r in range(2)]
    std = abs((f[0] - f[1]) / 2)
    x = (1 - std) * 100.0
    k = round(x)
    if std == 0.0 or abs(x - k) > ulps * math.ulp(x):
        return 0
    return 2 if x == k else (-1 if x < k else 1)


def near_integer_triples(seed: int = 5, n_random: int = 4000):
    """(alloc, req, pod) int64[n, 2] each whose (1 − std)·100 lies within 2 ulp of an integer: the fractions k / 1000
    against j / 1000 that do (a deterministic sweep), and those among n_random random triples over round capacities"""
    rng = np.random.default_rng(seed)
    out = []
    for a in range(0, 1001, 5):
        for b in range(0, 1001, 5):
            t = ((1000, 1000), (0, 0), (a, b))
            if near_integer(*t):
                out.append(t)
    caps_c = np.array([1000, 2000, 4000, 8000, 16000, 32000, 64000, 96000, 128000])
    caps_m = np.array([1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024]) * GI
    for _ in range(n_random):
        ac, am = int(rng.choice(caps_c)), int(rng.choice(caps_m))
        t = ((ac, am), (int(rng.integers(0, ac // 100 + 1)) * 100, int(rng.integers(0, am // (64 * MI) + 1)) * 64 * MI),
             (int(rng.integers(0, 41)) * 100, int(rng.integers(0, 65)) * 256 * MI))
        if near_integer(*t):
            out.append(t)
    arr = np.array(out, dtype=np.int64)
    return arr[:, 0], arr[:, 1], arr[:, 2]


def known_inputs():
    a = np.array([k[0] for k in KNOWN], dtype=np.int64)
    r = np.array([k[1] for k in KNOWN], dtype=np.int64)
    p = np.array([k[2] for k in KNOWN], dtype=np.int64)
    return a, r, p


# ---- the discriminating scenarios -----------------------------------------------------------------------------------
CPU_1, MEM_1 = 100, GI  # one percent of a scenario node


def pct2_pod(cpu_pct: int, mem_pct: int):
    return pod(cpu_pct * CPU_1, mem_pct * MEM_1)


def pct2_cluster(fills):
    """nodes of 10 cpu / 100 GiB, node i holding fills[i] = (cpu percent, memory percent) in one existing pod"""
    n = len(fills)
    nodes = np.repeat(F.make_node({"cpu": "10", "memory": "100Gi"}), n)
    metrics = np.repeat(F.make_node_metric(update_time_ns=synth.T0_NS, node_usage={"cpu": "0", "memory": "0"}), n)
    held = [(pct2_pod(*f), i) for i, f in enumerate(fills) if f != (0, 0)]
    return synth.Cluster(nodes, metrics, np.concatenate([p for p, _ in held]),
                         np.array([i for _, i in held], dtype=np.int32), synth.T0_NS + 10**9)


def scenario_config(s: Scenario, depth=2):
    prof = F.Profile(filter=(FIT,), score={BAL: 1})
    return F.build_config(profile=prof, batch_pods=s.batch, pods_per_wave=8, pipeline_depth=depth)


def scenario_listed():
    """Node 5 holds 10 % cpu / 60 % memory — low cpu, high memory — and the other 15 nodes 30 / 45.
    Pod 0 asks 40 / 0 (cpu-heavy): node 5 would hold 50 / 60 -> 100 - 50*0.10 = 95; the others 70 / 45 -> 87.5 -> 87.
    It goes to node 5.
    Pod 1 asks 10 / 0.  On the snapshot node 5 gives 20 / 60 -> 80 and is listed below every other node (40 / 45 ->
    97.5 -> 97).  After pod 0 it gives 60 / 60 -> 100: its key ROSE, and it is the sequential winner, though the first
    listed candidate, node 0, is unmodified — where the monotone rule stops."""
    fills = [(30, 45)] * 16
    fills[5] = (10, 60)
    return Scenario("listed", pct2_cluster(fills), np.concatenate([pct2_pod(40, 0), pct2_pod(10, 0)]), 2,
                    want_nodes=[5, 5], skip_differs_at=1)


def scenario_unlisted():
    """The same node raised by an in-flight round and in no list.  70 nodes hold 30 % cpu / 30 .. 39 % memory, node 70
    holds 0 / 80: for a pod of 10 / 0 it gives 10 / 80 -> 65, the last of 71 keys, so no record of 64 lists it (the
    others give 40 / 30 .. 39 -> 95 .. 99).  The round in flight put a pod of 70 / 0 on it (70 / 80): the 10 / 0 pod
    belongs there (80 / 80 -> 100), though its first listed candidate is untouched."""
    fills = [(30, 30 + (i % 10)) for i in range(70)] + [(0, 80)]
    return Scenario("unlisted", pct2_cluster(fills), np.concatenate([pct2_pod(10, 0), pct2_pod(70, 0)]), 1,
                    prev=[[(1, 70)]], want_nodes=[70], skip_differs_at=0)


SCENARIOS = {"listed": scenario_listed, "unlisted": scenario_unlisted}


# ---- the parity runs --------------------------------------------------------------------------------------------------
PROFILES = {
    "fit-la-bal-1-1-1": F.Profile(filter=(FIT, LA), score={FIT: 1, LA: 1, BAL: 1}),
    "balanced-only": F.Profile(filter=(FIT,), score={BAL: 3}),
    "fit-bal": F.Profile(filter=(FIT,), score={FIT: 1, BAL: 1}),
    "la-bal-1000": F.Profile(filter=(FIT, LA), score={LA: 1, BAL: 1000}),
}


def without_balanced(profile: str):
    p = PROFILES[profile]
    return F.Profile(filter=p.filter, score={k: v for k, v in p.score.items() if k != BAL})


def parity_config(profile: str, **kw):
    return F.build_config(profile=PROFILES[profile], **kw)


def rare_cluster():
    """300 nodes with rows outside the fast paths' domains: capacities at and past the bounds, an over-committed row,
    and rows whose cpu or memory allocatable is 0 (BalancedAllocation drops the resource there)"""
    cl = synth.make_cluster(300, seed=41)
    a = cl.nodes["allocatable"]
    a[10, abi.RES_CPU] = 1 << 24
    a[20, abi.RES_MEMORY] = 1 << 45
    a[30, abi.RES_CPU], a[30, abi.RES_MEMORY] = (1 << 24) + 5, (1 << 45) + 4096
    a[40, abi.RES_CPU], a[40, abi.RES_MEMORY] = 300, 512 * MI
    a[50, abi.RES_CPU] = 0
    a[60, abi.RES_MEMORY] = 0
    a[70, abi.RES_CPU], a[70, abi.RES_MEMORY] = 0, 0
    over = np.concatenate([pod(500, 1000 * MI)] * 5)  # 2500m / 5000 MiB requested on a 300m / 512 MiB node
    keep = ~np.isin(cl.existing_node, (40, 50, 60, 70))
    cl.existing_pods = np.concatenate([cl.existing_pods[keep], over])
    cl.existing_node = np.concatenate([cl.existing_node[keep], np.full(5, 40, np.int32)])
    return cl
