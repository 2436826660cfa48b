"""Inputs shared by tests/test_fit_strategy_rule.py (no GPU) and tests/test_fit_strategy_gpu.py — TEST INFRASTRUCTURE.

KNOWN: hand-derived answers of the MostAllocated rule, one node each.
scenario_a / _b / _c: the three situations in which a resolver that kept the monotone rule of DESIGN.md §3.3 answers
differently from sequential scheduling under MostAllocated.  Fill levels are in percent of a node of
10 cpu / 100 GiB, the same on both resources, so a node's MostAllocated score for a pod is its fill + the pod's."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from koordinator_amd import abi, framework, synth

F = framework
FIT, LA = F.NODE_RESOURCES_FIT, F.LOAD_AWARE
MI, GI = 1 << 20, 1 << 30


def pod(cpu_m: int, mem: int, **kw):
    req = {}
    if cpu_m:
        req["cpu"] = f"{cpu_m}m"
    if mem:
        req["memory"] = str(mem)
    return F.make_pod(req, **kw)


@dataclass
class Known:
    name: str
    alloc: tuple                    # (cpu milli, memory bytes)
    existing: list                  # [(cpu milli, memory bytes), ...] pods already on the node
    pod: tuple                      # the scored pod's requests
    weights: tuple = (1, 1)
    most: int = 0                   # the hand-derived MostAllocated score
    least: int | None = None        # and, where the case is about it, the LeastAllocated score of the same row
    fit_filter: bool = True
    why: str = ""


# Default non-zero request of a pod that requests nothing: 100m / 200 MiB.
KNOWN = [
    Known("quotients-truncate", (3000, 700 * MI), [(1000, 105 * MI)], (1000, 100 * MI), most=47,
          why="cpu 2000*100/3000 = 66.67 -> 66; memory 205*100/700 = 29.29 -> 29; (66 + 29)/2 = 47.5 -> 47"),
    Known("weights-3-1", (3000, 700 * MI), [(1000, 105 * MI)], (1000, 100 * MI), weights=(3, 1), most=56,
          why="(66*3 + 29*1)/4 = 56.75 -> 56"),
    Known("alloc-zero-drops-out", (3000, 0), [(1000, 0)], (1000, 0), weights=(3, 1), most=66,
          why="memory allocatable 0 leaves the weighted mean: 66*3/3 = 66 (not 66*3/4 = 49)"),
    Known("over-committed-100", (250, 1024 * MI), [(0, 0)] * 3, (0, 0), most=89, least=10,
          why="three zero-request pods hold 300m / 600 MiB non-zero; with the pod 400m > 250m: cpu 100 (LeastAllocated 0); "
              "memory 800*100/1024 = 78.1 -> 78 (LeastAllocated 224*100/1024 = 21.9 -> 21); (100 + 78)/2 = 89, (0 + 21)/2 = 10"),
    Known("requested-equals-capacity", (2000, 400 * MI), [(1000, 200 * MI)], (1000, 200 * MI), most=100, least=0,
          why="both quotients are exactly 100"),
    Known("zero-request-defaults", (1000, 1000 * MI), [], (0, 0), most=15,
          why="the pod scores by 100m / 200 MiB: cpu 10, memory 20; (10 + 20)/2 = 15"),
    Known("most-plus-least-is-99", (3000, 700 * MI), [(1000, 105 * MI)], (1000, 100 * MI), weights=(1, 0), most=66, least=33,
          why="cpu only: 2000*100/3000 -> 66 and 1000*100/3000 -> 33: the two strategies are not complements"),
]


def known_cluster(cases=KNOWN):
    """one node per case (node k = case k) with its existing pods; → (cluster, the scored pod of each case)"""
    nodes = np.concatenate([F.make_node({"cpu": f"{c.alloc[0]}m", "memory": str(c.alloc[1])}) for c in cases])
    metrics = np.repeat(F.make_node_metric(update_time_ns=synth.T0_NS, node_usage={"cpu": "0", "memory": "0"}), len(cases))
    ex = [(pod(*e), k) for k, c in enumerate(cases) for e in c.existing]
    pods = np.concatenate([p for p, _ in ex]) if ex else np.zeros(0, dtype=abi.POD_DTYPE)
    cl = synth.Cluster(nodes, metrics, pods, np.array([k for _, k in ex], dtype=np.int32), synth.T0_NS + 10**9)
    return cl, [pod(*c.pod) for c in cases]


def known_config(c: Known, strategy="MostAllocated", **kw):
    prof = F.Profile(filter=(FIT,), score={FIT: 1})
    return F.build_config(profile=prof, fit=F.NodeResourcesFitArgs({"cpu": c.weights[0], "memory": c.weights[1]}, strategy),
                          **kw)


# ---- the discriminating scenarios -----------------------------------------------------------------------------------
CPU_1, MEM_1 = 100, GI  # one percent of a scenario node


def pct_pod(p: int):
    return pod(p * CPU_1, p * MEM_1)


def pct_cluster(fills):
    """nodes of 10 cpu / 100 GiB, node i filled to fills[i] percent by one existing pod"""
    n = len(fills)
    nodes = np.repeat(F.make_node({"cpu": "10", "memory": "100Gi"}), n)
    metrics = np.repeat(F.make_node_metric(update_time_ns=synth.T0_NS, node_usage={"cpu": "0", "memory": "0"}), n)
    held = [(pct_pod(f), i) for i, f in enumerate(fills) if f]
    return synth.Cluster(nodes, metrics, np.concatenate([p for p, _ in held]),
                         np.array([i for _, i in held], dtype=np.int32), synth.T0_NS + 10**9)


@dataclass
class Scenario:
    name: str
    cl: object
    queue: np.ndarray               # the staged queue: the round's pods first, then the earlier rounds' pods
    nb: int                         # the round = queue[:nb]
    prev: list = field(default_factory=list)   # [[(queue index, node), ...]]: the in-flight rounds' placements
    batch: int = 32
    want_nodes: list = field(default_factory=list)  # the sequential winners, by hand
    skip_differs_at: int = 0        # the first pod the monotone rule answers differently


def scenario_config(s: Scenario, strategy="MostAllocated", depth=2):
    prof = F.Profile(filter=(FIT,), score={FIT: 1})
    return F.build_config(profile=prof, fit=F.NodeResourcesFitArgs(scoring_strategy=strategy), batch_pods=s.batch,
                          pods_per_wave=8, pipeline_depth=depth)


def scenario_a():
    """Node 3 is the fullest (60), node 7 the second (50), the rest hold 10.  A 45-percent pod does not fit node 3 and
    goes to node 7 (95).  The next pod, of 1 percent, lists the untouched node 3 first (61) — but node 7 now scores 96."""
    fills = [10] * 16
    fills[3], fills[7] = 60, 50
    return Scenario("a", pct_cluster(fills), np.concatenate([pct_pod(45), pct_pod(1)]), 2, want_nodes=[7, 7],
                    skip_differs_at=1)


def scenario_b():
    """70 nodes hold 50 .. 60 percent (node 0 the fullest), node 70 holds 5: for a 1-percent pod it is the last of 71
    keys, so no record of 64 lists it.  The round in flight put a 90-percent pod on it (95): the 1-percent pod belongs
    there (96), though its first listed candidate, node 0, is untouched."""
    fills = [60] + [50 + (i % 10) for i in range(1, 70)] + [5]
    return Scenario("b", pct_cluster(fills), np.concatenate([pct_pod(1), pct_pod(90)]), 1, prev=[[(1, 70)]],
                    want_nodes=[70], skip_differs_at=0)


def scenario_c():
    """64 nodes touched by the round in flight (slots 0 .. 63: node 0 holds 60, the others 20, each took a 1-percent
    pod), node 64 untouched at 55, nodes 65 .. 70 at 10.  Six 85-percent pods fit only on nodes 65 .. 70 and take one
    each (95): winners 65 .. 70 of the 70 distinct nodes, in slots 64 .. 69.  The seventh pod, of 1 percent, belongs on
    node 65 (96).  Its record starts node 0 (touched, slot 0), node 64 (untouched): one touched key above the best
    untouched one, and it is not a second-bank row — the monotone rule re-scores the first bank only and answers node 0."""
    fills = [60] + [20] * 63 + [55] + [10] * 6
    queue = np.concatenate([pct_pod(85)] * 6 + [pct_pod(1)] + [pct_pod(1)])
    return Scenario("c", pct_cluster(fills), queue, 7, prev=[[(7, i) for i in range(64)]], batch=64,
                    want_nodes=[65, 66, 67, 68, 69, 70, 65], skip_differs_at=6)


SCENARIOS = {"a": scenario_a, "b": scenario_b, "c": scenario_c}


# ---- the parity runs: synth clusters and queues ---------------------------------------------------------------------
SIZES = (1, 129, 1100, 16773)   # one lane, a partial tile, two tile groups, the size test_group_select uses
N_PODS = 400
BATCHES = (16, 38, 64)
DEPTHS = (1, 2, 3)
SEEDS = {1: 31, 129: 32, 1100: 33, 16773: 34}
PROFILES = {
    "fit-only": dict(profile=F.Profile(filter=(FIT,), score={FIT: 1})),
    "fit-la-1-1": dict(profile=F.Profile(filter=(FIT, LA), score={FIT: 1, LA: 1})),
    "prod-usage": dict(profile=F.Profile(filter=(FIT, LA), score={FIT: 1, LA: 1}),
                       la=F.LoadAwareSchedulingArgs(score_according_prod_usage=True)),
    "no-fit-filter": dict(profile=F.Profile(filter=(LA,), score={FIT: 1, LA: 1})),  # Fit scores rows it does not filter
}


def parity_config(profile: str, strategy="MostAllocated", **kw):
    return F.build_config(fit=F.NodeResourcesFitArgs(scoring_strategy=strategy), **PROFILES[profile], **kw)


def parity_queue(n_nodes: int, n_pods: int = N_PODS):
    """synth.make_pods, every fifth pod 24 times as large: 6 .. 192 cores and up to 768 GiB, which the fuller and the
    smaller nodes refuse (and, at the top of the range, every node: the largest holds 128 cores)"""
    pods = synth.make_pods(n_pods, seed=SEEDS[n_nodes] + 100)
    big = np.arange(n_pods) % 5 == 4
    for f in ("requests", "limits"):
        pods[f][big, abi.RES_CPU] *= 24
        pods[f][big, abi.RES_MEMORY] *= 24
    pods["nonzero_requests"][big] *= 24
    return pods


def parity_cluster(n_nodes: int):
    return synth.make_cluster(n_nodes, seed=SEEDS[n_nodes])


def aux_inputs(n_nodes: int = 1100):
    """the parity cluster with ephemeral-storage on 70 % of the nodes, and a queue where a third of the pods ask some"""
    rng = np.random.default_rng(77)
    cl = parity_cluster(n_nodes)
    cl.nodes["allocatable"][:, abi.RES_EPHEMERAL] = np.where(rng.random(n_nodes) < 0.7, rng.choice([100, 200, 400], n_nodes) * GI, 0)
    pods = parity_queue(n_nodes)
    k = rng.random(len(pods)) < 0.35
    pods["requests"][:, abi.RES_EPHEMERAL] = np.where(k, rng.choice([10, 50, 150, 500], len(pods)) * GI, 0)
    return cl, pods


def quota_inputs(n_nodes: int = 1100):
    cl, pods = parity_cluster(n_nodes), parity_queue(n_nodes)
    rng = np.random.default_rng(78)
    pods["quota_id"] = np.where(rng.random(len(pods)) < 0.8, rng.integers(1, 9, len(pods)), 0)
    pods["flags"] |= np.where(rng.random(len(pods)) < 0.2, abi.POD_NON_PREEMPTIBLE, 0)
    return cl, pods, synth.make_c5_quotas(pods, seed=79, n_quotas=8)


def assert_exercises(res, n_nodes: int, fit_filter: bool, what: str):
    """On the model's output alone: the input reaches the paths the comparison is about.  `res`: the model's Result with
    lead[b] for every batch size of BATCHES."""
    placed = res.node >= 0
    if n_nodes > 1:
        assert placed.sum() * 2 >= len(placed), f"{what}: {placed.sum()} of {len(placed)} pods placed"
        if fit_filter:  # without NodeResourcesFit's Filter nothing refuses a pod on these clusters
            assert (~placed).any(), f"{what}: no pod is unschedulable"
    else:
        # one node allows 110 pods: half of 400 cannot be placed there; some are, and with the Filter some are not
        assert placed.any() and (not fit_filter or (~placed).any()), what
    if n_nodes > 129:
        assert len(set(res.node[placed].tolist())) >= 8, f"{what}: {len(set(res.node[placed].tolist()))} distinct winners"
    if n_nodes > 1:
        # bin-packing's signature: the winner is a node an earlier pod of the queue went to, though another node led the
        # pod's keys when its round was evaluated
        for b in range(len(res.lead)):
            seen, hit = set(), 0
            for j in range(len(placed)):
                if placed[j]:
                    hit += int(res.node[j]) in seen and res.lead[b][j] != res.node[j]
                    seen.add(int(res.node[j]))
            assert hit >= 1, f"{what}: batch {BATCHES[b]}: no pod follows an earlier pod onto a node that did not lead"
