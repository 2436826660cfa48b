"""Checkers for what the round engine's wide pass and merge write (the record invariant) — TEST
INFRASTRUCTURE.

One checker per artefact, plain numpy over uint64, geometry from kg_debug_round_records' out_geom (a dict over
abi.DBG_GEOM_FIELDS); expected values come from oracle.node_keys and tests/round_model.py only.  A failed check raises
CheckFailed, an AssertionError that names the rule broken (`.rule`), so a test can tell which rule caught a fault:

  lists            list-zeros   a zero word before a non-zero one
                   list-set     the non-zero words are not the model's list for that node range
                   list-order   the right keys in the wrong order (tile lists: ascending node, group lists: descending key)
  record, against the pod's full key vector (no geometry)
                   order        keys not strictly descending, or a zero before a key
                   key-exact    a listed key is not the exact key of its node
                   prefix       the listed keys >= ub are not the first of the globally sorted feasible keys
                   ub-zero      ub == 0 although a feasible node is left out
                   ub-bound     a feasible node that is not listed has a key >= ub
  record, against the model for the geometry
                   ub-exact     ub differs from the model's
                   keys-exact   the keys >= ub differ from the model's keys >= ub
The exact part stops at ub on purpose: the per-wavefront merge drops keys below the full-list bound before it selects
and the per-block merge does not, so the two agree on ub and on the keys at or above it, and on nothing else.
"""
from __future__ import annotations

import numpy as np

import round_model

M32 = 0xFFFFFFFF


class CheckFailed(AssertionError):
    def __init__(self, rule: str, detail: str):
        super().__init__(f"[{rule}] {detail}")
        self.rule = rule


def key_node(k) -> int:
    return M32 - (int(k) & M32)


def make_key(score: int, node: int) -> int:
    return (int(score) << 32) | (M32 - int(node))


def check_lists(dev: np.ndarray, keys: np.ndarray, geom: dict, what: str = ""):
    """dev uint64[n_lists, list_len]: one pod's lists as the wide pass wrote them; keys: its oracle key vector."""
    dev = np.asarray(dev, dtype=np.uint64)
    want = round_model.round_lists(keys, geom)
    if dev.shape != want.shape:
        raise CheckFailed("list-set", f"{what}: {dev.shape[0]} lists of {dev.shape[1]}, the model has {want.shape}")
    bad = np.nonzero((dev != want).any(axis=1))[0]
    if not len(bad):
        return
    l = int(bad[0])
    span = geom["tile_nodes"] * (geom["group_tiles"] if geom["combined"] else 1)
    where = f"{what}: list {l} (nodes [{l * span}, {(l + 1) * span})), {len(bad)} lists differ"
    d, w = dev[l], want[l]
    nz = np.nonzero(d)[0]
    if len(nz) and nz[-1] != len(nz) - 1:
        raise CheckFailed("list-zeros", f"{where}: a zero before a key: {[hex(int(x)) for x in d]}")
    if set(d[d != 0].tolist()) != set(w[w != 0].tolist()):
        raise CheckFailed("list-set", f"{where}: got {[hex(int(x)) for x in d]}, want {[hex(int(x)) for x in w]}")
    raise CheckFailed("list-order", f"{where}: got {[hex(int(x)) for x in d]}, want {[hex(int(x)) for x in w]}")


def split_record(rec, kc: int):
    rec = np.asarray(rec, dtype=np.uint64)
    return rec[:kc], int(rec[kc])


def _check_order(top: np.ndarray, what: str) -> np.ndarray:
    """The record's non-zero keys, after checking that zeros come only at the tail and the keys strictly descend."""
    nz = np.nonzero(top)[0]
    n = len(nz)
    if n and nz[-1] != n - 1:
        raise CheckFailed("order", f"{what}: a zero before a key at position {int(np.nonzero(top == 0)[0][0])}")
    listed = top[:n]
    if n > 1 and not (listed[:-1] > listed[1:]).all():
        i = int(np.nonzero(~(listed[:-1] > listed[1:]))[0][0])
        raise CheckFailed("order", f"{what}: keys {i}, {i + 1} not strictly descending: {hex(int(listed[i]))}, "
                                   f"{hex(int(listed[i + 1]))}")
    return listed


def check_record(rec: np.ndarray, keys: np.ndarray, kc: int, what: str = ""):
    """The geometry-free part: rec uint64[kc + 1] (keys, ub) against the pod's full oracle key vector."""
    top, ub = split_record(rec, kc)
    keys = np.asarray(keys, dtype=np.uint64)
    listed = _check_order(top, what)
    n = len(listed)
    for i, k in enumerate(listed.tolist()):
        nd = key_node(k)
        if nd >= len(keys) or int(keys[nd]) != k:
            have = hex(int(keys[nd])) if nd < len(keys) else "no such node"
            raise CheckFailed("key-exact", f"{what}: position {i}: key {hex(k)} names node {nd}, whose key is {have}")
    feas = keys[keys != 0]
    ge = np.sort(feas[feas >= np.uint64(max(ub, 1))])[::-1]  # every feasible key >= ub, descending
    listed_ge = listed[listed >= np.uint64(ub)]
    m = len(listed_ge)
    if not np.array_equal(listed_ge, ge[:m]):
        i = int(np.nonzero(listed_ge != ge[:m])[0][0]) if len(ge) >= m else len(ge)
        raise CheckFailed("prefix", f"{what}: the {m} listed keys >= ub are not the {m} best feasible keys: first "
                                    f"difference at rank {i} (want node {key_node(ge[i]) if i < len(ge) else None})")
    if ub == 0 and len(feas) > n:
        raise CheckFailed("ub-zero", f"{what}: ub == 0 with {len(feas)} feasible nodes and {n} listed")
    if len(ge) > m:
        raise CheckFailed("ub-bound", f"{what}: node {key_node(ge[m])} is not listed and its key {hex(int(ge[m]))} "
                                      f">= ub {hex(ub)}")


def check_record_exact(rec: np.ndarray, model, kc: int, what: str = "", whole: bool = False, union=None):
    """The exact part: rec against the model's (top, ub) for the same lists.  whole: every key, not only those >= ub
    (the per-block merge of tile lists drops nothing).  union: the set of keys the lists held — with it, the keys below
    ub must at least come from the lists, in order (a check for callers that have no key vector)."""
    top, ub = split_record(rec, kc)
    mtop, mub = model
    if union is not None:
        for i, k in enumerate(_check_order(top, what).tolist()):
            if k not in union:
                raise CheckFailed("key-exact", f"{what}: position {i}: key {hex(k)} is in no list")
    if ub != mub:
        raise CheckFailed("ub-exact", f"{what}: ub {hex(ub)}, the model's {hex(mub)} "
                                      f"({'too small' if ub < mub else 'loose'})")
    got = [int(k) for k in top if k and (whole or int(k) >= ub)]
    want = [k for k in mtop if whole or k >= mub]
    if got != want:
        i = next((j for j, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise CheckFailed("keys-exact", f"{what}: {len(got)} keys{'' if whole else ' >= ub'}, the model has "
                                        f"{len(want)}; first difference at rank {i}")
