"""Inputs shared by tests/test_fit_shape_rule.py (no GPU) and tests/test_fit_shape_gpu.py — TEST INFRASTRUCTURE.

RAW: hand-derived values of the broken-linear function.  KNOWN: hand-derived node scores of the
RequestedToCapacityRatio rule, one node each.  scenario_below / scenario_unlisted: two situations specific to this
strategy in which a resolver that kept the monotone rule of DESIGN.md §3.3 answers differently from sequential
scheduling: an assume pushes one resource's shape value to 0, the resource leaves the weighted mean, and the node's key
goes UP."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import fit_shape_reference as R
from fit_strategy_cases import (BATCHES, DEPTHS, FIT, GI, LA, MI, PROFILES, SIZES, Scenario, aux_inputs,  # noqa: F401
                                known_cluster, parity_cluster, parity_queue, pod, quota_inputs)
from koordinator_amd import framework, synth

F = framework
RTCR = F.REQUESTED_TO_CAPACITY_RATIO
RISING, FALLING, PEAKED = R.RISING, R.FALLING, R.PEAKED
SHAPES = {"rising": RISING, "falling": FALLING, "peaked": PEAKED}
STEEP = [(0, 10), (3, 0)]
THREE = [(10, 2), (50, 8), (90, 4)]   # U[0] > 0 and U[n-1] < 100
KNEE = [(0, 0), (50, 10), (100, 3)]
HILL = [(0, 0), (40, 10), (80, 0)]    # 0 from 80 % on: a resource past it leaves the mean
ONE = [(40, 7)]
FULL = [(u, (u * 7) % 11) for u in range(101)]  # 101 points
TABLE_SHAPES = {"rising": RISING, "falling": FALLING, "peaked": PEAKED, "one-point": ONE, "101-points": FULL,
                "inner-points": THREE, "steep": STEEP, "knee": KNEE, "hill": HILL}

# (shape, p, raw(p), why)
RAW = [
    (STEEP, 1, 67, "100 + (-100*1)/3 = 100 + (-33) = 67: Go truncates -33.3 to -33 (floor division gives -34, 66)"),
    (STEEP, 2, 34, "100 + (-200)/3 = 100 - 66 = 34 (floor: 33)"),
    (STEEP, 3, 0, "on the last point"),
    (STEEP, 50, 0, "past the last point: S[n-1]"),
    (THREE, 5, 20, "before the first point: S[0]"),
    (THREE, 10, 20, "on the first point"),
    (THREE, 30, 50, "20 + 60*20/40 = 50"),
    (THREE, 33, 54, "20 + 60*23/40 = 20 + 34 (34.5 truncated) = 54"),
    (THREE, 50, 80, "on the middle point"),
    (THREE, 77, 53, "80 + (-40*27)/40 = 80 - 27 = 53"),
    (THREE, 71, 59, "80 + (-40*21)/40 = 80 + (-21) = 59"),
    (THREE, 90, 40, "on the last point"),
    (THREE, 95, 40, "past the last point"),
    (ONE, 0, 70, "a one-point shape is constant"),
    (ONE, 40, 70, "a one-point shape is constant"),
    (ONE, 100, 70, "a one-point shape is constant"),
    (THREE, -1, 20, "p < 0 reads lut[0]"),
    (FALLING, -7, 100, "p < 0 reads lut[0]"),
    (KNEE, 78, 61, "100 + (-70*28)/50 = 100 + (-39) = 61 (-39.2 truncated; floor gives -40, 60)"),
]


@dataclass
class Known:
    name: str
    shape: list
    alloc: tuple                    # (cpu milli, memory bytes)
    existing: list                  # [(cpu milli, memory bytes), ...] pods already on the node
    pod: tuple                      # the scored pod's requests
    weights: tuple = (1, 1)
    want: int = 0                   # the hand-derived score
    most: int | None = None         # where the case is about it: MostAllocated's score of the same row
    why: str = ""


# Default non-zero request of a pod that requests nothing: 100m / 200 MiB.
KNOWN = [
    Known("go-truncation", STEEP, (10000, 1000 * MI), [], (100, 10 * MI), weights=(1, 0), want=67,
          why="cpu 100*100/10000 = 1; raw(1) = 100 + (-100)/3 = 67 (floor division: 66)"),
    Known("round-half-away", RISING, (1000, 1000 * MI), [], (300, 450 * MI), want=38, most=37,
          why="identity shape: resource scores 30 and 45; 75/2 = 37.5 rounds to 38 (MostAllocated truncates to 37)"),
    Known("zero-score-leaves-the-mean", RISING, (20000, 1000 * MI), [], (0, 800 * MI), want=80, most=40,
          why="cpu 100*100/20000 = 0 -> raw 0: out of s and ws; memory 80; 80/1 = 80, not (0 + 80)/2 = 40"),
    Known("both-zero", FALLING, (1000, 1000 * MI), [], (1000, 1000 * MI), want=0,
          why="both utilizations 100, raw(100) = 0 twice: ws == 0 scores 0"),
    Known("alloc-zero-skipped", RISING, (3000, 0), [(1000, 0)], (1000, 0), weights=(3, 1), want=66,
          why="memory allocatable 0 takes no part: cpu 2000*100/3000 = 66.67 -> 66; 66*3/3 = 66 (not 66*3/4 = 49.5)"),
    Known("weight-zero-skipped", RISING, (1000, 1000 * MI), [], (300, 450 * MI), weights=(1, 0), want=30,
          why="memory weight 0 takes no part: 30/1 = 30"),
    Known("over-committed-reads-lut-100", KNEE, (250, 1024 * MI), [(0, 0)] * 3, (0, 0), want=46,
          why="three zero-request pods hold 300m / 600 MiB; with the pod 400m > 250m: u = 100, raw(100) = 30; memory "
              "800*100/1024 = 78, raw(78) = 61; (30 + 61)/2 = 45.5 rounds to 46"),
    Known("weights-3-1", KNEE, (3000, 700 * MI), [(1000, 105 * MI)], (1000, 100 * MI), weights=(3, 1), want=73,
          why="cpu u = 66: raw = 100 + (-70*16)/50 = 100 - 22 = 78; memory u = 29: raw = 100*29/50 = 58; "
              "(78*3 + 58)/4 = 292/4 = 73"),
]


def known_config(c: Known, **kw):
    """→ (config, NodeResourcesFitArgs): Fit alone, weight 1, the case's resource weights and shape"""
    prof = F.Profile(filter=(FIT,), score={FIT: 1})
    fit = F.NodeResourcesFitArgs({"cpu": c.weights[0], "memory": c.weights[1]}, RTCR, c.shape)
    return F.build_config(profile=prof, fit=fit, **kw), fit


# ---- the discriminating scenarios -----------------------------------------------------------------------------------
CPU_1, MEM_1 = 100, GI  # one percent of a scenario node (10 cpu / 100 GiB)


def pct_pod(c: int, m: int):
    return pod(c * CPU_1, m * MEM_1)


def pct_cluster(fills):
    """nodes of 10 cpu / 100 GiB, node i filled to fills[i] = (cpu percent, memory percent) by one existing pod"""
    sy = synth
    n = len(fills)
    nodes = np.repeat(F.make_node({"cpu": "10", "memory": "100Gi"}), n)
    metrics = np.repeat(F.make_node_metric(update_time_ns=sy.T0_NS, node_usage={"cpu": "0", "memory": "0"}), n)
    return sy.Cluster(nodes, metrics, np.concatenate([pct_pod(c, m) for c, m in fills]), np.arange(n, dtype=np.int32),
                      sy.T0_NS + 10**9)


SCENARIO_SHAPE = HILL  # raw(u) = 100u/40 up to 40, 100 - 100(u - 40)/40 up to 80 (truncating), 0 from 80 on


def scenario_config(s: Scenario, depth=2):
    prof = F.Profile(filter=(FIT,), score={FIT: 1})
    fit = F.NodeResourcesFitArgs(scoring_strategy=RTCR, shape=SCENARIO_SHAPE)
    return F.build_config(profile=prof, fit=fit, batch_pods=s.batch, pods_per_wave=8, pipeline_depth=depth), fit


def scenario_below():
    """Node 7 holds 70 % cpu / 30 % memory, node 3 holds 20 / 20, the rest 10 / 10.  Pod 0 (10 / 1) scores node 7 by
    memory alone — cpu 80 reads 0 and leaves the mean; memory 31 reads 77 — and goes there (node 3: (75 + 52)/2 = 63.5
    -> 64; the rest (50 + 27)/2 -> 39).  Pod 1 (1 / 1) was evaluated on the snapshot: node 3 first (52 and 52: 52), node
    7 second (cpu 71 reads 23, memory 31 reads 77: 50).  After pod 0 node 7 holds 80 / 31: for pod 1 cpu 81 reads 0 and
    drops out, memory 32 reads 80 — its key ROSE from 50 to 80 and beats node 3, though it is listed below it."""
    fills = [(10, 10)] * 16
    fills[3], fills[7] = (20, 20), (70, 30)
    return Scenario("below", pct_cluster(fills), np.concatenate([pct_pod(10, 1), pct_pod(1, 1)]), 2, want_nodes=[7, 7],
                    skip_differs_at=1)


def scenario_unlisted():
    """70 nodes hold 25 .. 29 % of both resources (a 1 / 1 pod scores them 65 .. 75, node 4 the best), node 70 holds
    70 / 30 and scores 50: the last of 71 keys, so no record of 64 lists it.  The round in flight put a 10 / 1 pod on it
    (80 / 31): the 1 / 1 pod now scores it 80 by memory alone and belongs there, though its first listed candidate is
    untouched."""
    fills = [(25 + i % 5, 25 + i % 5) for i in range(70)] + [(70, 30)]
    return Scenario("unlisted", pct_cluster(fills), np.concatenate([pct_pod(1, 1), pct_pod(10, 1)]), 1, prev=[[(1, 70)]],
                    want_nodes=[70], skip_differs_at=0)


SCENARIOS = {"below": scenario_below, "unlisted": scenario_unlisted}

# ---- the parity runs: fit_strategy_cases' synth clusters and queues -------------------------------------------------
# one profile and weight pair per shape, so that the three runs of a size differ in more than the table
PARITY = {
    "rising": dict(profile="fit-la-1-1", weights={"cpu": 1, "memory": 1}),
    "falling": dict(profile="prod-usage", weights={"cpu": 1, "memory": 2}),
    "peaked": dict(profile="fit-only", weights={"cpu": 3, "memory": 1}),
}


def parity_config(shape: str, **kw):
    """→ (config, NodeResourcesFitArgs)"""
    p = PARITY[shape]
    fit = F.NodeResourcesFitArgs(p["weights"], RTCR, SHAPES[shape])
    return F.build_config(fit=fit, **PROFILES[p["profile"]], **kw), fit


def assert_exercises(res, n_nodes: int, what: str):
    """On the model's output alone: the input reaches the paths the comparison is about (every parity profile has
    NodeResourcesFit's Filter, so some pods are refused)"""
    placed = res.node >= 0
    assert placed.any() and (~placed).any(), what
    if n_nodes > 1:
        assert placed.sum() * 2 >= len(placed), f"{what}: {placed.sum()} of {len(placed)} pods placed"
        nodes = res.node[placed].tolist()
        assert len(set(nodes)) < len(nodes), f"{what}: no node wins twice (no modified row ever wins)"
    if n_nodes > 129:
        assert len(set(res.node[placed].tolist())) >= 8, what
