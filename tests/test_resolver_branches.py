"""The round engine's resolver, branch by branch, against the plain model (DESIGN.md §4 "The resolver, branch by
branch").

resolve_round is driven through kg_debug_resolve: eval + merge on a snapshot, the earlier rounds' placements written
onto the table and into the modified-row lists, then the resolver exactly as a batch launches it — one call, one
stream, so which branch runs does not depend on timing.  Each scenario of tests/resolver_scenarios.py is built from the
records the device reports on the snapshot, and the model's census of it (tests/resolver_model.py: from the record and
the replay, never from the device) must contain the branch the scenario is named after; a scenario that misses its
branch fails with that message.  Every comparison is bit-exact: result keys, consumed / cursor / poison / CTL_SLOW, the
published list, the node-state columns and the quota rows against the model; on the 1,024- and 1,280-node tables also
every consumed key against the full sequential oracle, with no reference to the record."""
import numpy as np
import pytest

import resolver_model as RM
import resolver_scenarios as S
import round_model as M
from koordinator_amd import Engine, abi, framework
from koordinator_amd import synth
from koordinator_amd.abi import KoordGPUError
from oracle import oracle
from round_checks import key_node, make_key

pytestmark = pytest.mark.gpu
FIT, LA = framework.NODE_RESOURCES_FIT, framework.LOAD_AWARE
GI, MI = 1 << 30, 1 << 20
_tables = {}


def _table(name):
    if name not in _tables:
        _tables[name] = S.make_table(name)  # built once, shared, left unchanged
    return _tables[name]


def _consts(e):
    """The geometry constants, from the device: a stale call (poison set) runs nothing but the hook's plumbing."""
    d = e.debug_resolve(0, 1, poison=True)
    assert (d["consumed"], d["rounds"], d["n_list"]) == (0, 0, 0)
    return {k: d[k] for k in ("kc", "staged", "bank1_probe", "mod_hash", "score_bits", "depth")}


def _call(e, sit, n_quotas):
    dev = e.debug_resolve(sit.first, sit.nb, sit.prev, poison=sit.poison, cursor=sit.cursor)
    dev["state"] = e.read_state()
    dev["quotas"] = e.read_quotas(n_quotas) if n_quotas else None
    return dev


def _run(name, bits, sequential=True):
    table, kw, build, tags = S.SCENARIOS[name]
    cl, pods, quotas = _table(table)
    cfg = S._cfg(weights=S.WIDTHS[bits], **kw)
    with Engine(cfg, cl.n) as e:
        synth.load_into(e, cl)
        if quotas is not None:
            e.set_quotas(quotas)
        e.stage(pods)
        consts = _consts(e)
        if "profile" not in kw:
            assert consts["score_bits"] == bits
        b = S.Bench(cfg, cl, pods, quotas, records=lambda f, n: e.debug_round_records(f, n)[2], consts=consts)
        sit = build(b)
        assert len(sit.prev) <= consts["depth"] - 1
        snap = b.records(sit.first, sit.nb)
        dev = _call(e, sit, 0 if quotas is None else len(quotas))
        np.testing.assert_array_equal(dev["records"], snap, err_msg="the hook's records are not the snapshot's")
        rp = RM.replay(sit, dev["records"], consts["kc"])
        per_pod, rnd = RM.census(sit, rp, consts)
        got = RM.all_tags(per_pod, rnd)
        print(f"{name} bits {bits}: consumed {dev['consumed']}/{sit.nb}, CTL_SLOW {dev['slow']}, census {sorted(got)}")
        assert tags <= got, f"{name}: the situation does not select {sorted(tags - got)}: {[sorted(t) for t in per_pod]}"
        RM.check(dev, rp, f"{name}, score_bits {bits}")
        assert dev["seq"] == len(sit.prev) + 1  # the round published, stale or not
        if sequential:
            RM.check_sequential(sit, dev["out_keys"], dev["consumed"], name)
        if rp.poison and not sit.poison:
            # the next round starts at the cursor, on the fully written table: the stopped pod's answer is the oracle's
            nb2 = min(4, S.N_ROUND - rp.cursor)
            sit2 = RM.Situation(cfg, cl, rp.st, pods, rp.cursor, nb2, [], quotas=rp.quotas)
            dev2 = _call(e, sit2, 0 if quotas is None else len(quotas))
            rp2 = RM.replay(sit2, dev2["records"], consts["kc"])
            RM.check(dev2, rp2, f"{name}: the round after the stop")
            assert dev2["consumed"] >= 1
            RM.check_sequential(sit2, dev2["out_keys"], dev2["consumed"], f"{name}: the round after the stop")
    return sit, dev, rp


def _cases():
    return [pytest.param(n, b, id=f"{n}-bits{b}") for n, s in S.SCENARIOS.items() for b in S.WIDTHS
            if b == 13 or not ({"profile", "la"} & set(s[1]))]


@pytest.mark.parametrize("name,bits", _cases())
def test_resolver_branch(name, bits):
    sit, dev, rp = _run(name, bits)
    if name.startswith("stale"):
        # nothing but the sequence word changed: no key, no list, the table holds the interventions only
        assert (dev["out_keys"] == np.uint64(abi.DBG_RESOLVE_SENTINEL)).all() and dev["error"] == 0
        assert dev["poison"] == int(sit.poison) and dev["cursor"] == (sit.first if sit.cursor is None else sit.cursor)
    if name.startswith("stop"):
        assert (dev["out_keys"][dev["consumed"]:] == np.uint64(abi.DBG_RESOLVE_SENTINEL)).all()
        assert len(dev["list"]) == sum(1 for k in dev["out_keys"][:dev["consumed"]] if k)
    if name == "pend-rewin-shared":
        assert len(set(dev["list"].tolist())) == 1 and len(dev["list"]) == 3
    if name == "unschedulable":
        assert dev["out_keys"][1] == 0 and dev["out_keys"][0] != 0 and dev["out_keys"][2] != 0


@pytest.mark.parametrize("plugin", [framework.NODE_NUMA_RESOURCE, framework.DEVICE_SHARE, framework.RESERVATION])
def test_resolve_hook_refuses_other_profiles(plugin):
    prof = framework.Profile(filter=(FIT, LA, plugin), score={FIT: 1, LA: 1, plugin: 1})
    with Engine(framework.build_config(profile=prof), 64) as e:
        with pytest.raises(KoordGPUError) as err:
            e.debug_resolve(0, 1)
        assert err.value.code == abi.E_UNSUPPORTED


def test_resolve_hook_refuses_bad_input():
    cl, pods, _ = _table("plain")
    with Engine(S._cfg(batch=32, depth=2), cl.n) as e:
        synth.load_into(e, cl)
        e.stage(pods)
        before = e.read_state()
        for kw in (dict(first=len(pods) - 1, nb=2), dict(first=0, nb=33), dict(first=0, nb=1, prev=[[], []]),
                   dict(first=0, nb=1, prev=[[(0, cl.n)]]), dict(first=0, nb=1, prev=[[(len(pods), 0)]]),
                   dict(first=0, nb=1, prev=[[(0, 0)] * 33])):
            with pytest.raises(KoordGPUError) as err:
                e.debug_resolve(**kw)
            assert err.value.code == abi.E_INVALID, kw
        after = e.read_state()
        for k in before:
            np.testing.assert_array_equal(before[k], after[k], err_msg=f"{k}: a refused call changed the table")


# ---- the packed key's corner: the engine's largest table -------------------------------------------------------
N_MAX = 524_288


def _corner_table(big):
    """Every node alike and small, but the nodes `big`: empty and very large.  → (cluster, tool-and-probe pods)."""
    cl = M.tie_cluster(N_MAX)
    for i in big:
        cl.nodes["allocatable"][i, abi.RES_CPU], cl.nodes["allocatable"][i, abi.RES_MEMORY] = 1_000_000, 1024 * GI
    return cl


@pytest.mark.parametrize("node", [N_MAX - 1, 0], ids=["last-node", "node-0"])
def test_packed_key_corner_score_zero(node):
    """score_bits <= 13, a 524,288-node table, and a pod whose only feasible node is `node`, at total score 0, the row
    touched by an earlier round: the narrow key (score << 19 | 0x7FFFF − node) of score 0 on node 524,287 is 0, which
    the wave maximum reads as "no key".  The sequential answer places the pod there.  A Fit-only score: the node's
    requested + the pod's request equal its allocatable, so both least-requested terms are 0."""
    cl = _corner_table([node])
    cfg = S._cfg(profile=framework.Profile(score={FIT: 40}), batch=16, depth=2)
    tiny = S._pod(1, MI)
    fill = S._pod(1_000_000 - 1, 1024 * GI - MI)  # with `tiny` on the node: exactly its allocatable
    small = S._pod(1_000, GI)
    pods = np.concatenate([fill, small, small, tiny])
    with Engine(cfg, cl.n) as e:
        synth.load_into(e, cl)
        e.stage(pods)
        consts = _consts(e)
        assert consts["score_bits"] <= 13
        b = S.Bench(cfg, cl, pods, records=lambda f, n: e.debug_round_records(f, n)[2], consts=consts)
        sit = b.sit(3, [[(3, node)]])
        dev = _call(e, sit, 0)
    rp = RM.replay(sit, dev["records"], consts["kc"])
    # the case is the case it claims to be, from the oracle alone
    st = rp.st_pre
    kv = oracle.node_keys(cfg, cl.nodes, cl.metrics, st, pods[0], cl.now_ns, 0, cl.n)
    assert np.count_nonzero(kv) == 1 and int(kv[node]) == make_key(0, node), hex(int(kv[node]))
    assert rp.out_keys[0] == make_key(0, node) and rp.trace[0]["from_touched"] and rp.consumed == 3
    print(f"corner node {node}: device key {hex(int(dev['out_keys'][0]))}, the model's {hex(rp.out_keys[0])}")
    RM.check(dev, rp, f"score 0 on touched node {node}")


def test_packed_key_corner_top_tie():
    """The other end of the narrow key, at weights 40 + 41 (score_bits 13): touched node 0 and touched node 524,287
    tie on the highest score the table holds, and the lower index wins.  (The width's largest total, 8,100, needs both
    plugins at 100, which no node reaches once a pod has been assumed on it — a touched row never scores it; the tie
    is at the largest score these rows do reach, printed below.)"""
    cl = _corner_table([0, N_MAX - 1])
    cfg = S._cfg(weights=(40, 41), batch=16, depth=2)
    pods = np.concatenate([S._pod(1_000, GI), S._pod(1_000, GI), S._pod(1, MI)])
    with Engine(cfg, cl.n) as e:
        synth.load_into(e, cl)
        e.stage(pods)
        consts = _consts(e)
        assert consts["score_bits"] == 13
        b = S.Bench(cfg, cl, pods, records=lambda f, n: e.debug_round_records(f, n)[2], consts=consts)
        sit = b.sit(2, [[(2, N_MAX - 1), (2, 0)]])
        dev = _call(e, sit, 0)
    rp = RM.replay(sit, dev["records"], consts["kc"])
    t = rp.trace[0]
    assert t["tkeys"][0] >> 32 == t["tkeys"][N_MAX - 1] >> 32 == t["best"] >> 32 and t["winner"] == 0, t["tkeys"]
    print(f"top tie: score {t['best'] >> 32} on nodes 0 and {N_MAX - 1}")
    RM.check(dev, rp, "tie between touched nodes 0 and 524,287")
