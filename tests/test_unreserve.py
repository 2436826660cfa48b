"""Unreserve and the scheduler clock in the GPU snapshot cache.

kg_pods_unreserve is the framework's Unreserve of placed pods (every enabled plugin's Unreserve: NodeInfo + LoadAware
assign cache, NodeNUMAResource Release, DeviceShare updateCacheUsed(add=false), Reservation forgetPod, ElasticQuota
UnreservePod); or_unreserve is its oracle.  kg_engine_set_clock moves the clock isNodeMetricExpired reads
(loadaware/helper.go:36-41 calls time.Since on every Filter/Score).

CPU: the oracle's Unreserve of every placed pod restores the initial state exactly.  GPU: schedule → Unreserve a
subset → schedule more, interleaved identically on the engine and the oracle, bit-exact (placements, totals, cpusets,
NUMA / GPU / reservation / quota state); and expiry re-evaluated when the clock moves between calls."""
import numpy as np
import pytest

import test_parity_gpu as TP
from koordinator_amd import Engine, abi, framework as F, synth
from oracle import oracle

NUMA_PROFILE = F.Profile(filter=(F.NODE_RESOURCES_FIT, F.LOAD_AWARE, F.NODE_NUMA_RESOURCE),
                         score={F.NODE_RESOURCES_FIT: 1, F.LOAD_AWARE: 1, F.NODE_NUMA_RESOURCE: 1})
C5_PROFILE = F.Profile(filter=(F.NODE_RESOURCES_FIT, F.LOAD_AWARE, F.RESERVATION, F.DEVICE_SHARE),
                       score={F.NODE_RESOURCES_FIT: 1, F.LOAD_AWARE: 1, F.RESERVATION: 5000, F.DEVICE_SHARE: 1})


def _st(cfg, cluster):
    st = oracle.states(cluster.n)
    oracle.add_pods(cfg, st, cluster.existing_pods, cluster.existing_node)
    return st


def _c5(n_nodes, n_pods, seed):
    cluster, dev, rsv = synth.make_c5_cluster(n_nodes, seed=seed)
    pods = synth.make_c5_pods(n_pods, seed=seed + 1)
    quotas = synth.make_c5_quotas(pods, seed=seed + 2)
    return cluster, dev, rsv, pods, quotas


# ---- CPU: the oracle's Unreserve inverts Reserve --------------------------------------------------------------
def test_oracle_unreserve_numa_restores_state():
    cfg = F.build_config(profile=NUMA_PROFILE)
    cluster, numa = synth.make_numa_cluster(120, seed=501)
    pods = synth.make_numa_pods(600, seed=502)
    st = _st(cfg, cluster)
    st0 = st.copy()
    buf = oracle.numa_states(numa)
    buf0 = buf.copy()
    node, _, cpus, _, nalloc = oracle.schedule_full(cfg, cluster.nodes, cluster.metrics, st, pods, cluster.now_ns, 4,
                                                    numa_buf=buf, with_numa_alloc=True)
    assert (node >= 0).sum() > 100 and (nalloc[:, 0] != 0).any()
    for j in np.nonzero(node >= 0)[0][::-1]:
        oracle.unreserve(cfg, st, pods[j], node[j], numa_buf=buf, cpus=cpus[j], numa_alloc=nalloc[j])
    assert np.array_equal(st, st0)
    assert np.array_equal(oracle.numa_state_read(buf, cluster.n)[0], oracle.numa_state_read(buf0, cluster.n)[0])
    for a, b in zip(oracle.numa_state_read(buf, cluster.n)[1:], oracle.numa_state_read(buf0, cluster.n)[1:]):
        assert np.array_equal(a, b)


def test_oracle_unreserve_c5_restores_state():
    cfg = F.build_config(profile=C5_PROFILE)
    cluster, dev, rsv, pods, quotas = _c5(150, 700, 511)
    st = _st(cfg, cluster)
    st0, d, r, q = st.copy(), dev.copy(), rsv.copy(), quotas.copy()
    node, _, slot, minors = oracle.schedule_resv(cfg, cluster.nodes, cluster.metrics, st, r, pods, cluster.now_ns,
                                                 devices=d, quotas=q, n_threads=4, with_minors=True)
    assert (slot >= 0).any() and (minors != 0).any()
    for j in np.nonzero(node >= 0)[0]:
        oracle.unreserve(cfg, st, pods[j], node[j], devices=d, rsv=r, quotas=q, minors=minors[j], slot=slot[j])
    assert np.array_equal(st, st0)
    for k in ("used_core", "used_memory", "used_ratio"):
        assert np.array_equal(d[k], dev[k]), k
    for k in ("allocated_cpu", "allocated_mem", "assigned"):
        assert np.array_equal(r[k], rsv[k]), k
    assert np.array_equal(q["used"], quotas["used"]) and np.array_equal(q["non_preemptible_used"],
                                                                        quotas["non_preemptible_used"])


# ---- GPU: interleaved schedule / Unreserve / schedule -----------------------------------------------------------
def _subset(node, k):
    """Every k-th placed pod of the chunk, as a mask over it."""
    placed = np.nonzero(node >= 0)[0]
    m = np.zeros(len(node), dtype=bool)
    m[placed[::k]] = True
    return m


@pytest.mark.gpu
def test_unreserve_fit_loadaware_quota_interleaved():
    cfg = F.build_config(batch_pods=32, pods_per_wave=8)
    cluster = synth.make_cluster(1500, seed=521)
    pods = synth.make_pods(4000, seed=522)
    rng = np.random.default_rng(523)
    pods["quota_id"] = np.where(rng.random(len(pods)) < 0.7, rng.integers(1, 4, len(pods)), 0)
    quotas = np.zeros(3, dtype=abi.QUOTA_DTYPE)
    quotas["used_limit"] = -1
    quotas["min"] = -1
    quotas["used_limit"][:, 0] = pods["requests"][:, 0].sum() // 5
    st, q = _st(cfg, cluster), quotas.copy()
    a, b = 2000, len(pods)
    w1, ws1, _, _ = oracle.schedule_full(cfg, cluster.nodes, cluster.metrics, st, pods[:a], cluster.now_ns, 8, quotas=q)
    m = _subset(w1, 3)
    for j in np.nonzero(m)[0]:
        oracle.unreserve(cfg, st, pods[j], w1[j], quotas=q)
    w2, ws2, _, _ = oracle.schedule_full(cfg, cluster.nodes, cluster.metrics, st, pods[a:], cluster.now_ns, 8, quotas=q)
    with Engine(cfg, cluster.n) as e:
        synth.load_into(e, cluster)
        e.set_quotas(quotas)
        e.stage(pods)
        e.schedule_staged(0, a)
        g1, _ = e.fetch(0, a)
        assert np.array_equal(g1, w1)
        e.unreserve(0, a, m)
        e.unreserve(0, a, m)  # a second Unreserve of the same pods is a no-op
        g1b, _ = e.fetch(0, a)
        assert np.array_equal(g1b, np.where(m, -1, w1))
        e.schedule_staged(a, b - a)
        g2, gs2 = e.fetch(a, b - a)
        assert np.array_equal(g2, w2) and np.array_equal(gs2, ws2)
        TP._assert_state_equal(e, st)
        assert np.array_equal(e.read_quotas(len(quotas)), q)


@pytest.mark.gpu
def test_unreserve_numa_interleaved():
    cfg = F.build_config(profile=NUMA_PROFILE, batch_pods=16, pods_per_wave=1)
    cluster, numa = synth.make_numa_cluster(400, seed=531)
    pods = synth.make_numa_pods(2000, seed=532)
    st, buf = _st(cfg, cluster), oracle.numa_states(numa)
    a = 1000
    w1, _, c1, _, n1 = oracle.schedule_full(cfg, cluster.nodes, cluster.metrics, st, pods[:a], cluster.now_ns, 8,
                                            numa_buf=buf, with_numa_alloc=True)
    m = _subset(w1, 2)
    for j in np.nonzero(m)[0]:
        oracle.unreserve(cfg, st, pods[j], w1[j], numa_buf=buf, cpus=c1[j], numa_alloc=n1[j])
    w2, ws2, c2, _ = oracle.schedule_full(cfg, cluster.nodes, cluster.metrics, st, pods[a:], cluster.now_ns, 8,
                                          numa_buf=buf)
    with Engine(cfg, cluster.n) as e:
        synth.load_numa_into(e, cluster, numa)
        e.stage(pods)
        e.schedule_staged(0, a)
        g1, _ = e.fetch(0, a)
        assert np.array_equal(g1, w1) and np.array_equal(e.fetch_cpusets(0, a), c1)
        e.unreserve(0, a, m)
        e.schedule_staged(a, len(pods) - a)
        g2, gs2 = e.fetch(a, len(pods) - a)
        assert np.array_equal(g2, w2) and np.array_equal(gs2, ws2)
        assert np.array_equal(e.fetch_cpusets(a, len(pods) - a), c2)
        ga, gc, gm = e.read_numa()
        wa, wc, wm = oracle.numa_state_read(buf, cluster.n)
        assert np.array_equal(ga, wa) and np.array_equal(gc, wc) and np.array_equal(gm, wm)
        TP._assert_state_equal(e, st)


@pytest.mark.gpu
def test_unreserve_c5_interleaved():
    cfg = F.build_config(profile=C5_PROFILE)
    cluster, dev, rsv, pods, quotas = _c5(600, 2400, 541)
    st, d, r, q = _st(cfg, cluster), dev.copy(), rsv.copy(), quotas.copy()
    a = 1200
    w1, _, s1, m1 = oracle.schedule_resv(cfg, cluster.nodes, cluster.metrics, st, r, pods[:a], cluster.now_ns,
                                         devices=d, quotas=q, n_threads=8, with_minors=True)
    m = _subset(w1, 2)
    for j in np.nonzero(m)[0]:
        oracle.unreserve(cfg, st, pods[j], w1[j], devices=d, rsv=r, quotas=q, minors=m1[j], slot=s1[j])
    assert (m & (s1 >= 0)).any() and (m & (m1 != 0)).any()
    w2, ws2, s2, m2 = oracle.schedule_resv(cfg, cluster.nodes, cluster.metrics, st, r, pods[a:], cluster.now_ns,
                                           devices=d, quotas=q, n_threads=8, with_minors=True)
    with Engine(cfg, cluster.n) as e:
        synth.load_c5_into(e, cluster, dev, rsv, quotas)
        e.stage(pods)
        e.schedule_staged(0, a)
        g1, _ = e.fetch(0, a)
        assert np.array_equal(g1, w1) and np.array_equal(e.fetch_reservations(0, a), s1)
        e.unreserve(0, a, m)
        assert np.array_equal(e.fetch_reservations(0, a), np.where(m, -1, s1))
        e.schedule_staged(a, len(pods) - a)
        g2, gs2 = e.fetch(a, len(pods) - a)
        assert np.array_equal(g2, w2) and np.array_equal(gs2, ws2)
        assert np.array_equal(e.fetch_reservations(a, len(pods) - a), s2)
        assert np.array_equal(e.fetch_devices(a, len(pods) - a), m2)
        uc, um, ur = e.read_devices()
        assert np.array_equal(uc, d["used_core"]) and np.array_equal(um, d["used_memory"])
        assert np.array_equal(ur, d["used_ratio"])
        ac, am, asg = e.read_reservations()
        on = np.arange(abi.MAX_RSV_SLOTS)[None, :] < r["n"][:, None]
        assert np.array_equal(ac, np.where(on, r["allocated_cpu"], 0))
        assert np.array_equal(am, np.where(on, r["allocated_mem"], 0))
        assert np.array_equal(asg, np.where(on, r["assigned"], 0))
        assert np.array_equal(e.read_quotas(len(quotas)), q)
        TP._assert_state_equal(e, st)


@pytest.mark.gpu
def test_metric_expiry_follows_the_clock():
    """Metrics updated 0–300 s before T0: as the clock moves from T0+10 s to T0+100 s and T0+400 s between calls,
    more nodes' NodeMetric expires (180 s): LoadAware Filter lets them through and scores them 0."""
    cfg = F.build_config()
    cluster = synth.make_cluster(1000, seed=551)
    rng = np.random.default_rng(552)
    has = cluster.metrics["has_update_time"].astype(bool)
    t0 = int(cluster.metrics["update_time_unix_nano"][has][0])
    cluster.metrics["update_time_unix_nano"] = np.where(has, t0 - rng.integers(0, 300, cluster.n) * 10**9, 0)
    pods = synth.make_pods(3000, seed=553)
    nows = [cluster.now_ns, t0 + 100 * 10**9, t0 + 400 * 10**9]
    st = _st(cfg, cluster)
    want = [oracle.schedule(cfg, cluster.nodes, cluster.metrics, st, pods[k * 1000:(k + 1) * 1000], nows[k], 8)
            for k in range(3)]
    with Engine(cfg, cluster.n) as e:
        synth.load_into(e, cluster)
        e.stage(pods)
        for k in range(3):
            if k:
                e.set_clock(nows[k])
            e.schedule_staged(k * 1000, 1000)
            node, score = e.fetch(k * 1000, 1000)
            assert np.array_equal(node, want[k][0]) and np.array_equal(score, want[k][1]), k
    # the clock mattered: the same queue at a frozen clock places differently
    st2 = _st(cfg, cluster)
    frozen = oracle.schedule(cfg, cluster.nodes, cluster.metrics, st2, pods, nows[0], 8)[0]
    assert not np.array_equal(frozen[1000:], np.concatenate([want[1][0], want[2][0]]))
