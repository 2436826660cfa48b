"""kg_pods_pick_candidate / kg_pods_preempt on the device against tests/pick_reference.py (upstream's
pickOneNodeForPreemption as narrowing passes; validated by hand-derived cases in test_preempt_pick_rule.py) and, end to
end, against oracle.select_victims per candidate followed by that reference.  Bar: the whole kg_preempt_pick record and
the victim list, equal.

The reduction-shape cases are built so that the reference alone reaches every rule (test_cases_reach_every_rule checks
that without a device): per candidate count, `level` cases perturb one template in the dimension of one rule, and
`planted` cases put a winner that exactly one rule decides at a chosen position."""
from functools import lru_cache

import numpy as np
import pytest

from koordinator_amd import Engine, abi, framework as F, synth
from koordinator_amd.abi import KoordGPUError
from oracle import oracle
from pick_reference import pick_candidate
from test_preemption import RSV_ONLY, _random_candidates, _with_ephemeral
from test_reservation_oracle import PROFILE

I32_MIN, I32_MAX = -2**31, 2**31 - 1
COUNTS = (1, 2, 63, 64, 65, 257, 4097)   # one lane, the wave edge, the block edge, several partials
LENS = (0, 1, 2, 63, 64, 65, 130)        # segment lengths: empty, below / at / past one wave step, three steps
PRIOS = np.array([I32_MIN, -1, 0, 100, I32_MAX], dtype=np.int32)
STARTS = np.array([0, 16 * 10**17, 16 * 10**17 + 1, 17 * 10**17], dtype=np.int64)
LATER = 18 * 10**17                      # later than every value of STARTS
REJECTS = np.array([abi.REJECT_FIT_CPU, abi.REJECT_NO_VICTIMS, abi.REJECT_LOADAWARE | abi.REJECT_FIT_MEMORY], dtype=np.int32)


def _template(rng, first_prios=PRIOS):
    """one victim list: (kept, priority, start) with at least one victim kept"""
    n = int(rng.choice(LENS[1:]))
    kept = (rng.random(n) < 0.6).astype(np.uint8)
    if not kept.any():
        kept[int(rng.integers(0, n))] = 1
    prio = rng.choice(PRIOS, n)
    prio[int(np.argmax(kept))] = rng.choice(first_prios)
    return kept, prio, rng.choice(STARTS, n)


def _append(t, prio, start):
    return (np.append(t[0], np.uint8(1)), np.append(t[1], np.int32(prio)), np.append(t[2], np.int64(start)))


def _assemble(lists, nvio, reject):
    off = np.zeros(len(lists) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(t[0]) for t in lists])
    cat = lambda q, dt: np.concatenate([t[q] for t in lists]).astype(dt) if off[-1] else np.zeros(0, dtype=dt)  # noqa: E731
    nodes = np.arange(len(lists), dtype=np.int32)[::-1].copy()  # node index != position
    return (nodes, off, np.asarray(reject, dtype=np.int32), cat(0, np.uint8), np.asarray(nvio, dtype=np.int32),
            cat(1, np.int32), cat(2, np.int64))


def _reject(rng, nc):
    """about a third of the candidates ineligible"""
    return np.where(rng.random(nc) < 1 / 3, rng.choice(REJECTS, nc), 0).astype(np.int32)


def level_case(rng, nc, level):
    """level 0: everything random, empty and fully reprieved segments included.  level L >= 1: every candidate is one
    template with the dimensions of the rules before L left alone and those of rule L and the later ones drawn at
    random (1 the violations, 2 the first victim's priority, 3 the others' priorities, 4 extra victims that add 0 to
    the sum, 5 the start times; 6 nothing), so the candidates tie up to rule L and the later rules see real variety."""
    lists, nvio = [], []
    base = _template(rng)
    base_nvio = int(rng.integers(0, 2))
    for _ in range(nc):
        if level == 0:
            n = int(rng.choice(LENS))
            t = ((rng.random(n) < 0.5).astype(np.uint8), rng.choice(PRIOS, n), rng.choice(STARTS, n))
            nvio.append(int(rng.integers(0, min(2, int(t[0].sum())) + 1)))
            lists.append(t)
            continue
        kept, prio, start = (a.copy() for a in base)
        first = int(np.argmax(kept))
        nv = base_nvio
        if level <= 1:
            nv = int(rng.integers(0, min(2, int(kept.sum())) + 1))
        if level <= 2:
            prio[first] = rng.choice(PRIOS)
        if level <= 3:
            others = np.nonzero(kept)[0][1:]
            prio[others] = rng.choice(PRIOS, len(others))
        if level <= 4:
            for _ in range(int(rng.integers(0, 3))):
                kept, prio, start = _append((kept, prio, start), I32_MIN, rng.choice(STARTS))
        if level <= 5:
            start = rng.choice(STARTS, len(start))
        lists.append((kept, prio, start))
        nvio.append(nv)
    return _assemble(lists, nvio, _reject(rng, nc))


def planted_case(rng, nc, w, rule):
    """every candidate the same list; the one at position w differs so that exactly `rule` prefers it (rule 6: the
    candidates in front of it are ineligible)"""
    base = _template(rng, first_prios=PRIOS[1:])
    others, win, o_nvio, w_nvio = base, base, 1, 1
    if rule == 0:
        win = (np.zeros_like(base[0]), base[1], base[2])  # every potential victim reprieved
    elif rule == 1:
        w_nvio = 0
    elif rule == 2:
        p = base[1].copy()
        p[int(np.argmax(base[0]))] = I32_MIN
        win = (base[0], p, base[2])
    elif rule == 3:
        others, win = _append(base, 100, STARTS[1]), _append(base, 0, STARTS[1])
    elif rule == 4:
        others, win = _append(_append(base, I32_MIN, STARTS[1]), I32_MIN, STARTS[1]), _append(base, I32_MIN, STARTS[1])
    elif rule == 5:
        win = (base[0], base[1], np.full_like(base[2], LATER))
    reject = _reject(rng, nc)
    if rule == 6:
        reject[:w] = abi.REJECT_FIT_CPU
    reject[w] = 0
    lists = [others] * nc
    lists[w] = win
    nvio = np.full(nc, o_nvio)
    nvio[w] = w_nvio
    return _assemble(lists, nvio, reject)


def _positions(nc):
    """position 0, the last one, just past a wave and just past a block"""
    return sorted({0, nc - 1} | {p for p in (64, 256) if p < nc})


@lru_cache(maxsize=None)
def cases(nc):
    """[(name, arrays, reference Pick, the rule the case was built for or None)] — built once, shared, never modified"""
    rng = np.random.default_rng(5000 + nc)
    out = []
    for level in range(7):
        a = level_case(rng, nc, level)
        out.append((f"level{level}", a, pick_candidate(*a), None))
    for w in _positions(nc):
        for rule in range(7):
            a = planted_case(rng, nc, w, rule)
            out.append((f"planted{w}/rule{rule}", a, pick_candidate(*a), (w, rule)))
    return out


def test_cases_reach_every_rule():
    """CPU: the reference alone reaches every rule on the parameter set, each planted winner is where it was put and
    won by the rule it was built for, and about a third of the candidates is ineligible."""
    decided = set()
    for nc in COUNTS:
        mine = set()
        for name, a, ref, planted in cases(nc):
            mine.add(ref.rule)
            if planted:
                w, rule = planted
                assert ref.candidate == w, (nc, name)
                # a single eligible candidate returns at upstream's first check (rule 1), whatever it was planted for
                assert ref.rule == (rule if ref.eligible > 1 or rule == 0 else 1), (nc, name, ref.rule)
        if nc >= 63:
            assert mine >= set(range(7)), (nc, mine)
        decided |= mine
    assert decided >= set(range(7)), decided
    rej = np.concatenate([a[2] for _, a, _, p in cases(4097) if p is None])
    assert 0.25 < (rej != 0).mean() < 0.42


def _same(pick, victims, ref, where):
    assert tuple(int(pick[k]) for k in abi.PREEMPT_PICK_DTYPE.names) == ref.record(), (where, pick, ref)
    assert victims.tolist() == ref.victims, where


@pytest.mark.gpu
@pytest.mark.parametrize("nc", COUNTS)
def test_pick_candidate_reduction_shapes(nc):
    """kg_pods_pick_candidate on synthetic arrays: the whole record and the victim list equal the reference's for every
    level and every planted winner, and every rule decided at least one case (from two candidates on; one candidate
    alone can only be decided by rule 0 or upstream's first check)."""
    cfg = F.build_config()
    decided = set()
    with Engine(cfg, 4097) as e:
        e.upsert_nodes(synth.make_cluster(4097, seed=11).nodes)
        for name, a, ref, _ in cases(nc):
            pick, victims = e.pick_candidate(*a)
            _same(pick, victims, ref, (nc, name))
            decided.add(ref.rule)
        # the same call twice: the scratch is reused, the answer is the same
        name, a, ref, _ = cases(nc)[0]
        _same(*e.pick_candidate(*a), ref, (nc, name, "again"))
    assert decided >= (set(range(7)) if nc >= 63 else {0, 1}), decided


def _priorities(rng, vics):
    return ([rng.choice(np.array([0, 100, 1000], dtype=np.int32), len(v)) for v in vics],
            [rng.choice(STARTS, len(v)) for v in vics])


def _flat(off, per_node, dtype):
    return np.concatenate([np.asarray(v, dtype=dtype) for v in per_node]) if off[-1] else np.zeros(0, dtype=dtype)


def _e2e_pods(rng, seed):
    """12 Reservation-queue pods, half with ephemeral-storage; eight of them asking 24 to 96 cores, so that most
    candidates have to give up victims; and one pod no node can hold"""
    pods = synth.make_rsv_pods(12, seed=960 + seed)
    em = rng.random(len(pods)) < 0.5
    pods["requests"][em, abi.RES_EPHEMERAL] = rng.integers(1, 40, int(em.sum())) * 10**9
    big = np.arange(len(pods)) >= 4
    cpu = rng.choice(np.array([24, 48, 64, 96], dtype=np.int64), len(pods)) * 1000
    giant = np.append(big, True)
    pods = np.concatenate([pods, pods[:1]])
    cpu = np.append(cpu, 10**7)  # 10,000 cores: fits nowhere, whatever is preempted
    for field in ("requests", "limits", "nonzero_requests"):
        col = 0 if field == "nonzero_requests" else abi.RES_CPU
        pods[field][giant, col] = cpu[giant]
    return pods


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2])
def test_preempt_matches_oracle_and_reference(seed):
    """kg_pods_preempt over 48 candidates of the 96-node Reservation cluster of
    test_device_select_victims_matches_oracle (random victim orders, slots, PDB flags; both profiles), with priorities
    from {0, 100, 1000} and start times from a small set: the pick, the victims and the status words equal
    oracle.select_victims per candidate followed by the reference pick.  Among 48 random nodes some hold the pod without
    preemption and rule 0 picks one, so each pod is also run over the candidates PostFilter would pass — the ones that
    need victims or fail — where the other rules decide.  A pod no node can hold makes "none" occur."""
    rng = np.random.default_rng(170 + seed)
    cluster, rsv = synth.make_rsv_cluster(96, seed=910 + seed)
    cluster = _with_ephemeral(cluster, rng)
    pods = _e2e_pods(rng, seed)
    seen = {"picked": 0, "none": 0, "victims": 0, "no preemption needed": 0}
    for prof in (RSV_ONLY, PROFILE):
        cfg = F.build_config(profile=prof)
        st = oracle.states(cluster.n)
        oracle.add_pods(cfg, st, cluster.existing_pods, cluster.existing_node)
        with Engine(cfg, cluster.n) as e:
            synth.load_rsv_into(e, cluster, rsv)
            for j in range(len(pods)):
                nodes, vics, slots, viol = _random_candidates(cluster, rsv, rng, 48)
                prios, starts = _priorities(rng, vics)
                want = [oracle.select_victims(cfg, cluster.nodes[i], cluster.metrics[i], st[i:i + 1], rsv[i],
                                              pods[j:j + 1], vics[c], slots[c], viol[c], cluster.now_ns)
                        for c, i in enumerate(nodes)]
                needs = [c for c, (r, k, _) in enumerate(want) if r != 0 or np.any(k)]
                for sel in (list(range(len(nodes))), needs):
                    sub = lambda per: [per[c] for c in sel]  # noqa: E731
                    off = np.zeros(len(sel) + 1, dtype=np.int64)
                    off[1:] = np.cumsum([len(vics[c]) for c in sel])
                    ref = pick_candidate(nodes[sel], off, [want[c][0] for c in sel],
                                         _flat(off, [np.asarray(want[c][1], dtype=np.uint8) for c in sel], np.uint8),
                                         [want[c][2] for c in sel], _flat(off, sub(prios), np.int32),
                                         _flat(off, sub(starts), np.int64))
                    pick, victims, rej = e.preempt(pods[j:j + 1], nodes[sel], sub(vics), sub(prios), sub(starts),
                                                   sub(slots), sub(viol), want_reject=True)
                    assert rej.tolist() == [int(want[c][0]) for c in sel], (prof, j)
                    assert tuple(int(pick[k]) for k in abi.PREEMPT_PICK_DTYPE.names) == ref.record(), (prof, j, pick, ref)
                    assert victims.tolist() == [k - int(off[ref.candidate]) for k in ref.victims], (prof, j)
                    seen["none" if ref.candidate < 0 else "picked"] += 1
                    seen["victims"] += ref.n_victims
                    seen["no preemption needed"] += ref.rule == 0
    assert all(v > 0 for v in seen.values()), seen


@lru_cache(maxsize=None)
def _cluster_10k():
    cluster = synth.make_cluster(10000, seed=4242)
    order = np.argsort(cluster.existing_node, kind="stable")
    bounds = np.searchsorted(cluster.existing_node[order], np.arange(cluster.n + 1))
    vics = [cluster.existing_pods[order[bounds[i]:bounds[i + 1]]] for i in range(cluster.n)]
    rng = np.random.default_rng(4244)
    prios, starts = _priorities(rng, vics)
    return cluster, vics, prios, starts


@pytest.mark.gpu
def test_preempt_fused_equals_unfused_10k_nodes():
    """Every node of the 10k-node Fit + LoadAware cluster a candidate, its pods the potential victims: kg_pods_preempt
    equals kg_pods_pick_candidate over what kg_pods_select_victims returned, and both equal the reference over the
    same.  Thousands of these nodes hold the pod without preemption (rule 0 takes the first), so the same is done over
    the nodes PostFilter would pass, the ones that need victims or fail, where the winner has victims.
    Scheduler.select_candidate returns the winner's pod records."""
    cluster, all_vics, all_prios, all_starts = _cluster_10k()
    cfg = F.build_config()
    s = F.Scheduler(cfg, cluster.n)
    with_victims = 0
    try:
        e = s.engine
        synth.load_into(e, cluster)
        pod = F.make_pod(requests={"cpu": "24", "memory": "48Gi"})
        nodes = np.arange(cluster.n, dtype=np.int32)
        for _ in range(2):
            vics, prios, starts = ([per[i] for i in nodes] for per in (all_vics, all_prios, all_starts))
            off = np.zeros(len(nodes) + 1, dtype=np.int64)
            off[1:] = np.cumsum([len(v) for v in vics])
            fp, fs = _flat(off, prios, np.int32), _flat(off, starts, np.int64)
            rej, kept, nvio = e.select_victims(pod, nodes, vics)
            fk = _flat(off, kept, np.uint8)
            ref = pick_candidate(nodes, off, rej, fk, nvio, fp, fs)
            assert ref.candidate >= 0 and ref.eligible == int((rej == 0).sum())
            unfused, u_vic = e.pick_candidate(nodes, off, rej, fk, nvio, fp, fs)
            _same(unfused, u_vic, ref, "unfused")
            fused, f_vic, f_rej = e.preempt(pod, nodes, vics, prios, starts, want_reject=True)
            assert fused.tolist() == unfused.tolist() and np.array_equal(f_rej, rej)
            assert (f_vic + off[ref.candidate]).tolist() == ref.victims
            pick, pods = s.select_candidate(pod, nodes, vics, prios, starts)
            assert pick.tolist() == fused.tolist()
            assert pods.tobytes() == vics[ref.candidate][f_vic].tobytes() and len(pods) == ref.n_victims
            with_victims += ref.n_victims > 0
            nodes = nodes[(rej != 0) | np.array([k.any() for k in kept])]
            assert 100 < len(nodes) < cluster.n
    finally:
        s.close()
    assert with_victims == 1


@pytest.mark.gpu
def test_preempt_refusals_arguments_and_state():
    cluster = synth.make_cluster(300, seed=77)
    cfg = F.build_config()
    pod = F.make_pod(requests={"cpu": "24", "memory": "48Gi"})
    nodes = np.arange(40, dtype=np.int32)
    vics = [cluster.existing_pods[cluster.existing_node == i] for i in nodes]
    rng = np.random.default_rng(78)
    prios, starts = _priorities(rng, vics)
    longest = max(len(v) for v in vics)
    assert longest >= 2
    with Engine(cfg, cluster.n) as e:
        synth.load_into(e, cluster)
        before = e.read_state()
        pick, victims, rej = e.preempt(pod, nodes, vics, prios, starts, want_reject=True)
        off = np.zeros(len(nodes) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(v) for v in vics])
        s_rej, s_kept, s_nvio = e.select_victims(pod, nodes, vics)
        assert np.array_equal(rej, s_rej) and int(pick["eligible"]) == int((s_rej == 0).sum())
        # victims_cap below the longest segment: refused before any launch, by both entry points
        for call in (lambda: e.preempt(pod, nodes, vics, prios, starts, victims_cap=longest - 1),
                     lambda: e.pick_candidate(nodes, off, s_rej, _flat(off, s_kept, np.uint8), s_nvio,
                                              _flat(off, prios, np.int32), _flat(off, starts, np.int64),
                                              victims_cap=longest - 1)):
            with pytest.raises(KoordGPUError) as ei:
                call()
            assert ei.value.code == abi.E_INVALID and "victims_cap" in str(ei.value)
        # the exact cap passes
        again, v2 = e.preempt(pod, nodes, vics, prios, starts, victims_cap=longest)
        assert again.tolist() == pick.tolist() and v2.tolist() == victims.tolist()
        # no candidates: "none"
        for none, v in (e.preempt(pod, nodes[:0], [], [], []),
                        e.pick_candidate(nodes[:0], np.zeros(1, np.int64), [], [], [], [], [])):
            assert tuple(int(none[k]) for k in abi.PREEMPT_PICK_DTYPE.names) == (-1, -1, 0, 0, 0, 0, 0, 0) and len(v) == 0
        # argument errors of the dry run are the pick's too
        with pytest.raises(KoordGPUError) as ei:
            e.preempt(pod, np.array([cluster.n], dtype=np.int32), vics[:1], prios[:1], starts[:1])
        assert ei.value.code == abi.E_INVALID and "node index" in str(ei.value)
        with pytest.raises(KoordGPUError) as ei:
            e.pick_candidate(nodes[:1], np.zeros(2, np.int64), [0], [], [-1], [], [])
        assert ei.value.code == abi.E_INVALID and "num_violating" in str(ei.value)
        gpu_pod = pod.copy()
        gpu_pod["device_requests"][0, 0] = 100  # device requests without DeviceShare: kg_pods_select_victims refuses
        for call in (lambda: e.select_victims(gpu_pod, nodes, vics), lambda: e.preempt(gpu_pod, nodes, vics, prios, starts)):
            with pytest.raises(KoordGPUError) as ei:
                call()
            assert ei.value.code == abi.E_UNSUPPORTED and "DeviceShare" in str(ei.value)
        # nothing was assumed: the engine's state is what it was, and it still schedules
        after = e.read_state()
        assert all(np.array_equal(before[k], after[k]) for k in before)
        assert e.select_victims(pod, nodes, vics)[0].tolist() == s_rej.tolist()
    # a profile kg_pods_select_victims refuses is refused
    prof = F.Profile(filter=(F.NODE_RESOURCES_FIT, F.LOAD_AWARE, F.POD_TOPOLOGY_SPREAD),
                     score={F.NODE_RESOURCES_FIT: 1, F.LOAD_AWARE: 1, F.POD_TOPOLOGY_SPREAD: 2})
    with Engine(F.build_config(profile=prof), cluster.n) as e:
        synth.load_into(e, cluster)
        for call in (lambda: e.select_victims(pod, nodes, vics), lambda: e.preempt(pod, nodes, vics, prios, starts)):
            with pytest.raises(KoordGPUError) as ei:
                call()
            assert ei.value.code == abi.E_UNSUPPORTED and "PodTopologySpread" in str(ei.value)
