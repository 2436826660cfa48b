"""Situations that put the round engine's resolver on one branch each (DESIGN.md §4 "The resolver, branch by
branch") — TEST INFRASTRUCTURE, shared by tests/test_resolver_model.py (records from tests/round_model.py, no GPU) and
tests/test_resolver_branches.py (records from the device).

A scenario is built adaptively: it reads the round's records on the snapshot first and chooses the earlier rounds'
placements from them.  `SCENARIOS[name] = (table, config, builder, tags)`: the builder returns a Situation, and the
model's census of it must contain `tags` — the branch the scenario is named after."""
from __future__ import annotations

import numpy as np

import resolver_model as RM
import round_model as M
from koordinator_amd import abi, framework, synth
from oracle import oracle
from round_checks import key_node

FIT, LA = framework.NODE_RESOURCES_FIT, framework.LOAD_AWARE
GI, MI = 1 << 30, 1 << 20
CONSTS = {"kc": 64, "staged": 3, "bank1_probe": 8, "mod_hash": 512}  # the CPU runs' geometry; the GPU runs read theirs
TILE = 128          # nodes per tile of the model geometry (the clone tables keep every tile's list short of full)
N_ROUND = 64        # the queue: N_ROUND round pods, then the tool pods below
TINY, BIG, HUGE_TOOL, AUX_TOOL = N_ROUND, N_ROUND + 1, N_ROUND + 2, N_ROUND + 3


def _pod(cpu, mem, eph=0, quota_id=0):
    p = synth.make_pods(1, seed=3)
    p["requests"][0, :] = 0
    p["requests"][0, abi.RES_CPU], p["requests"][0, abi.RES_MEMORY] = cpu, mem
    p["requests"][0, abi.RES_EPHEMERAL] = eph
    p["limits"][0] = p["requests"][0]
    p["nonzero_requests"][0] = (cpu, mem)
    p["quota_id"] = quota_id
    return p


def _tools(huge_cpu=200_000):
    return np.concatenate([_pod(1, MI), _pod(16_000, 32 * GI), _pod(huge_cpu, GI), _pod(1, MI, eph=90 * GI)])


# ---- tables -----------------------------------------------------------------------------------------------------
def plain_table(n=1024, seed=41):
    cl = synth.make_cluster(n, seed=seed)
    cl.nodes["allocatable"][:, abi.RES_EPHEMERAL] = 400 * GI
    return cl, np.concatenate([synth.make_pods(N_ROUND, seed=seed + 1), _tools()])


def clone_table(n_clones, n=1280, seed=43, eph=0, pod_eph=0):
    """A synth table plus n_clones identical, empty, very large nodes, at most 7 per tile (so no tile's list is full
    and ub comes from the record alone); the round's pods fit on the clones only."""
    cl = synth.make_cluster(n, seed=seed)
    per = 7 if n_clones > 9 else 9  # ≤ 9 clones: one tile, whose list is then full (the early-stop tables)
    idx = np.array([t * TILE + k for t in range(n // TILE) for k in range(per)][:n_clones])
    nd = cl.nodes
    nd["allocatable"][idx] = 0
    nd["allocatable"][idx, abi.RES_CPU], nd["allocatable"][idx, abi.RES_MEMORY] = 2_000_000, 4096 * GI
    nd["allocatable"][idx, abi.RES_EPHEMERAL] = eph
    nd["flags"][idx] = abi.NODE_VALID
    nd["custom_usage_thresholds"][idx] = -1
    cl.metrics[idx] = cl.metrics[idx[0]]
    cl.metrics["node_usage"][idx] = 0
    keep = ~np.isin(cl.existing_node, idx)
    cl.existing_pods, cl.existing_node = cl.existing_pods[keep], cl.existing_node[keep]
    pods = np.concatenate([_pod(200_000, GI, eph=pod_eph) for _ in range(N_ROUND)] + [_tools()])
    return cl, pods, idx


def rare_table(seed=47):
    """No Fit filter, LoadAware outweighs Fit: node 5 is large, empty and idle, and the round's pods carry a non-zero
    request far above what LoadAware estimates for them, so they pile onto node 5 past its capacity — assume on the
    touched row leaves the fast evaluation's exact domain while the node keeps winning."""
    cl = synth.make_cluster(1024, seed=seed)
    cl.nodes["allocatable"][5, abi.RES_CPU], cl.nodes["allocatable"][5, abi.RES_MEMORY] = 128_000, 1024 * GI
    cl.nodes["flags"][5] = abi.NODE_VALID
    cl.nodes["custom_usage_thresholds"][5] = -1
    cl.metrics["node_usage"][5] = 0
    keep = cl.existing_node != 5
    cl.existing_pods, cl.existing_node = cl.existing_pods[keep], cl.existing_node[keep]
    pod = _pod(100, 256 * MI)
    pod["nonzero_requests"][0, 0] = 50_000
    return cl, np.concatenate([np.concatenate([pod] * N_ROUND), _tools()])


# ---- the bench: a table, its queue and a source of records ----------------------------------------------------------
class Bench:
    def __init__(self, cfg, cl, pods, quotas=None, records=None, consts=None):
        self.cfg, self.cl, self.pods, self.quotas = cfg, cl, pods, quotas
        self.st0 = oracle.states(cl.n)
        if len(cl.existing_pods):
            oracle.add_pods(cfg, self.st0, cl.existing_pods, cl.existing_node)
        self.consts = dict(CONSTS) if consts is None else consts
        self._records = records or self._model_records

    def _model_records(self, first, nb):
        cl, kc = self.cl, self.consts["kc"]
        geom = M.model_geometry(cl.n, tile_nodes=TILE, kc=kc)
        out = np.zeros((nb, kc + 1), dtype=np.uint64)
        for j in range(nb):
            kv = oracle.node_keys(self.cfg, cl.nodes, cl.metrics, self.st0, self.pods[first + j], cl.now_ns, 0, cl.n)
            top, ub = M.round_record(kv, geom)[1]
            out[j, :len(top)], out[j, kc] = top, ub
        return out

    def records(self, first, nb):
        return self._records(first, nb)

    def listed(self, rec):
        return [key_node(k) for k in rec[:self.consts["kc"]] if k]

    def unlisted(self, recs, count, avoid=()):
        """`count` valid nodes no record of the round lists: touching them leaves every pod on its fast path."""
        seen = {key_node(k) for r in recs for k in r[:self.consts["kc"]] if k} | set(avoid)
        ok = [i for i in range(self.cl.n) if i not in seen and self.cl.nodes["flags"][i] & abi.NODE_VALID]
        assert len(ok) >= count
        return ok[:count]

    def sit(self, nb, prev=(), first=0, **kw):
        return RM.Situation(self.cfg, self.cl, self.st0, self.pods, first, nb, [list(l) for l in prev], **kw)

    def drops(self, pod, node, below, tool=BIG, most=8):
        """How many `tool` pods on `node` put its key for `pod` below the key `below` (the state is left alone)."""
        st = self.st0.copy()
        for c in range(1, most + 1):
            oracle.apply_pod(self.cfg, st, self.pods[tool], node, +1)
            sit = self.sit(1)
            if RM.key_now(sit, st, pod, node) < below:
                return c
        raise AssertionError(f"node {node} stays above {hex(below)} after {most} pods")


def _fill(nodes, tool=TINY):
    return [(tool, int(n)) for n in nodes]


# ---- builders: bench → Situation --------------------------------------------------------------------------------
def fast_empty(b):
    return b.sit(1)


def fast_touched(b):
    recs = b.records(0, 8)
    return b.sit(8, [_fill(b.unlisted(recs, 5))])


def slow_e_wins(b):
    recs = b.records(0, 4)
    top = b.listed(recs[0])
    return b.sit(4, [[(BIG, top[0])] * b.drops(b.pods[0], top[0], int(recs[0][1]))])


def touched_wins(b, fillers=0):
    """Pod 0's best listed node, barely touched, behind `fillers` untouched-by-any-record nodes: bank fillers // 64."""
    recs = b.records(0, 4)
    fill = b.unlisted(recs, fillers)
    prev = [_fill(fill[i:i + 32]) for i in range(0, fillers, 32)] + [[(TINY, b.listed(recs[0])[0])]]
    return b.sit(4, prev)


def touched_wins_bank1(b):
    return touched_wins(b, 64)


def tie(b, cross):
    """Ten clones, all touched: eight heavily, two barely and alike — they tie at the top; the lower index wins."""
    clones = b.listed(b.records(0, 1)[0])
    assert len(clones) == 10
    a, c = clones[2], clones[6]
    heavy = [(HUGE_TOOL, n) for n in clones if n not in (a, c)]
    if cross:
        pad = _fill(b.unlisted(b.records(0, 1), 56))
        prev = [[(TINY, c)] + heavy + pad[:23], pad[23:55], [(TINY, a)]]  # c in slot 0, a in slot 64
    else:
        prev = [[(TINY, c), (TINY, a)] + heavy]
    return b.sit(2, prev)


def tie_same_bank(b):
    return tie(b, False)


def tie_cross_bank(b):
    return tie(b, True)


def last_w_fresh(b):
    return b.sit(6)


def last_w_touched(b):
    recs = b.records(0, 6)
    return b.sit(6, [[(TINY, b.listed(recs[0])[0])]])


def pend_hbm(b):
    """Pod 0's three best listed nodes dropped below its fourth: it wins the fourth fresh, at position kStaged."""
    recs = b.records(0, 4)
    top, ks = b.listed(recs[0]), b.consts["staged"]
    prev = []
    for q in range(ks):
        prev += [(BIG, top[q])] * b.drops(b.pods[0], top[q], int(recs[0][ks]))
    assert len(prev) <= 32
    return b.sit(4, [prev])


def one_clone_three_pods(b):
    return b.sit(3)


def prev_total(b, counts):
    recs = b.records(0, 4)
    fill = b.unlisted(recs, sum(counts))
    prev, k = [], 0
    for c in counts:
        prev.append(_fill(fill[k:k + c]))
        k += c
    prev[0][0] = (TINY, b.listed(recs[0])[0])  # slot 0: pod 0 takes the slow path
    return b.sit(4, prev)


def fresh_run(b, fillers):
    """64 pods, each taking a fresh clone, behind `fillers` earlier placements: slots fillers .. fillers + 63."""
    recs = b.records(0, 1)
    return b.sit(64, [_fill(b.unlisted(recs, fillers))] if fillers else [])


def dup_lists(b):
    recs = b.records(0, 4)
    f = b.unlisted(recs, 8)
    top = b.listed(recs[0])[0]
    return b.sit(4, [_fill([top, f[0], top, f[1]]), [], _fill([f[0], f[2], top])])


def hash_chain(b):
    """Three touched nodes with one mod_hash value: a probe chain of three.  The hash is computed here only to choose
    the nodes and to assert the chain; no expected value uses it."""
    recs = b.records(0, 4)
    bits = int(np.log2(b.consts["mod_hash"]))
    buckets = {}
    for n in b.unlisted(recs, 600):
        buckets.setdefault(((n * 2654435761) & 0xFFFFFFFF) >> (32 - bits), []).append(n)
    chain = next(v for v in buckets.values() if len(v) >= 3)[:3]
    assert len({((n * 2654435761) & 0xFFFFFFFF) >> (32 - bits) for n in chain}) == 1
    return b.sit(4, [_fill([b.listed(recs[0])[0]] + chain)])


def stop(b, nb, touch=0):
    """Nine clones in one tile: the list holds eight, ub is the eighth's key.  Pod j takes clone j; the eighth pod
    meets best == ub; the ninth finds nothing it may take.  touch: clones the earlier round already took."""
    clones = b.listed(b.records(0, 1)[0])
    return b.sit(nb, [[(HUGE_TOOL, n) for n in clones[:touch]]] if touch else [])


def unschedulable(b):
    return b.sit(3)


def quota_round(b):
    return b.sit(5, [[(TINY, b.listed(b.records(0, 1)[0])[0])]], quotas=b.quotas)


def aux_table(b):
    return b.sit(2, [[(AUX_TOOL, b.listed(b.records(0, 1)[0])[0])]])


def aux_round(b):
    return b.sit(3)


def rare(b):
    return b.sit(8)


def mixed(b):
    recs = b.records(0, 8)
    t0, t1 = b.listed(recs[0])[0], b.listed(recs[2])[1]
    return b.sit(8, [[(TINY, t0)] + [(BIG, t1)] * 3])


def stale_poison(b):
    return b.sit(4, [[(TINY, 3)]], poison=True)


def stale_cursor(b):
    return b.sit(4, [[(TINY, 3)]], first=4, cursor=2)


# ---- benches by table -------------------------------------------------------------------------------------------
def _cfg(weights=(40, 41), batch=32, depth=4, profile=None, **kw):
    prof = profile or framework.Profile(score={FIT: weights[0], LA: weights[1]})
    return framework.build_config(profile=prof, batch_pods=batch, pods_per_wave=8, pipeline_depth=depth, **kw)


def make_table(table):
    """→ (cluster, queue, quotas or None) of a named table (built once per test module and left unchanged)."""
    quotas = None
    if table == "plain":
        cl, pods = plain_table()
    elif table == "unsched":
        cl, pods = plain_table()
        pods[1] = _pod(10_000_000, GI)[0]
    elif table == "quota":
        cl, pods = plain_table()
        pods["quota_id"][:5] = (1, 1, 1, 0, 2)
        quotas = np.zeros(2, dtype=abi.QUOTA_DTYPE)
        quotas["used_limit"], quotas["min"] = -1, -1
        quotas["used_limit"][0, 0] = int(pods["requests"][:2, abi.RES_CPU].sum())  # the third pod finds it spent
        quotas["used_limit"][1, 0] = 1_000_000
    elif table == "rare":
        cl, pods = rare_table()
    elif table.startswith("clones"):
        n = int(table[6:].split("-")[0])
        eph, pod_eph = (100 * GI, 20 * GI) if table.endswith("-auxt") else (100 * GI, 60 * GI) if table.endswith("-auxr") else (0, 0)
        cl, pods, _ = clone_table(n, eph=eph, pod_eph=pod_eph)
    else:
        raise KeyError(table)
    return cl, pods, quotas


NO_FIT_FILTER = framework.Profile(filter=(LA,), score={FIT: 1, LA: 41})
# name → (table, config keywords, builder, tags the census must contain)
SCENARIOS = {
    "fast-empty": ("plain", {}, fast_empty, {"fast-empty", "pend-never"}),
    "fast-touched": ("plain", {}, fast_touched, {"fast"}),
    "slow-e-wins": ("plain", {}, slow_e_wins, {"slow-e-wins"}),
    "touched-wins-bank0": ("plain", {}, touched_wins, {"slow-touched-wins", "win-bank0"}),
    "touched-wins-bank1": ("plain", {}, touched_wins_bank1, {"slow-touched-wins", "win-bank1", "probe-hit"}),
    "tie-same-bank": ("clones10", {}, tie_same_bank, {"tie-touched", "win-bank0"}),
    "tie-cross-bank": ("clones10", {}, tie_cross_bank, {"tie-touched", "tie-cross-bank"}),
    "last_w-fresh": ("plain", {}, last_w_fresh, {"last_w-fresh", "pend-staged"}),
    "last_w-touched": ("plain", {}, last_w_touched, {"last_w-touched"}),
    "pend-hbm": ("plain", {}, pend_hbm, {"pend-hbm"}),
    "pend-rewin-shared": ("clones1", {}, one_clone_three_pods, {"pend-rewin-twice", "shared-winner-3"}),
    "prev-63": ("plain", {}, lambda b: prev_total(b, (32, 31)), {"prev-total-63", "slow-touched-wins"}),
    "prev-64": ("plain", {}, lambda b: prev_total(b, (32, 32)), {"prev-total-64", "slow-touched-wins"}),
    "prev-65": ("plain", {}, lambda b: prev_total(b, (32, 32, 1)), {"prev-total-65", "probe-miss"}),
    "prev-96": ("plain", {}, lambda b: prev_total(b, (32, 32, 32)), {"prev-total-96", "probe-miss"}),
    "slots-60-123": ("clones70", {"batch": 64, "depth": 2}, lambda b: fresh_run(b, 60),
                     {"prev-total-60", "slot-63", "slot-64", "probe-hit", "probe-past"}),
    "slots-64-127": ("clones70", {"batch": 64, "depth": 2}, lambda b: fresh_run(b, 64),
                     {"prev-total-64", "slot-127", "probe-hit", "probe-past"}),
    "dup-lists": ("plain", {}, dup_lists, {"dup-in-list", "dup-across-lists", "empty-list-between"}),
    "hash-chain": ("plain", {}, hash_chain, {"prev-total-4"}),
    "stop-at-0": ("clones9", {}, lambda b: stop(b, 4, touch=8), {"stop-at-0"}),
    "stop-middle": ("clones9", {}, lambda b: stop(b, 12), {"stop-middle", "best-eq-ub"}),
    "stop-last": ("clones9", {}, lambda b: stop(b, 9), {"stop-last", "best-eq-ub"}),
    "unschedulable": ("unsched", {}, unschedulable, {"unschedulable", "unsched-inside"}),
    "quota": ("quota", {}, quota_round, {"quota-reject", "quota-exhausted-in-round"}),
    "aux-table": ("clones1-auxt", {}, aux_table, {"aux-reject-table"}),
    "aux-round": ("clones1-auxr", {}, aux_round, {"aux-reject-round"}),
    "rare-touched": ("rare", {"profile": NO_FIT_FILTER}, rare, {"over-capacity-touched"}),
    "fit-only-score": ("plain", {"profile": framework.Profile(score={FIT: 40})}, mixed, {"slow-touched-wins"}),
    "la-only-score": ("plain", {"profile": framework.Profile(score={LA: 41})}, mixed, {"slow-touched-wins"}),
    "prod-usage-score": ("plain", {"la": framework.LoadAwareSchedulingArgs(score_according_prod_usage=True)}, mixed,
                         {"slow-touched-wins"}),
    "default-weights": ("plain", {"profile": framework.Profile()}, mixed, {"slow-touched-wins"}),
    "stale-poison": ("plain", {}, stale_poison, {"stale"}),
    "stale-cursor": ("plain", {}, stale_cursor, {"stale"}),
}
WIDTHS = {13: (40, 41), 14: (41, 41)}
# every branch of the issue's list, by the tag that proves it was selected
BRANCHES = set().union(*(s[3] for s in SCENARIOS.values()))
