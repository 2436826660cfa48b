"""The schedule calls of tests/test_round_stats.py, shared with the recorder tests/golden/make_round_stats.py: per
case the kg_stats of one kg_pods_schedule call.

The parity tests compare placements, which cannot tell one diagnostic word of the round engine's control blocks from
another (csrc/round_ctl.h: pods re-scored on the chain, the reserved word, rounds run, pods consumed).  kg_stats carries
those words to the host, so the cases pin them.  Every case is 300 nodes and 600 pods at batch 16, pipeline depth 1:
no wide pass overlaps a resolver, so the rounds, their early stops and the counts are deterministic.

  fit_la         NodeResourcesFit + LoadAware                       resolve_round<.., false>
  fit_la_quota   the same with an ElasticQuota table that runs out  resolve_round<.., true>
  numa           + NodeNUMAResource                                 resolve_round_numa2
  deviceshare    + DeviceShare                                      resolve_round_ds
  exact          + Reservation, 600 pods                            the batched exact rounds (rounds-run word)
  exact_3        the same table, 3 pods                             the per-pod exact pass"""
import numpy as np

from koordinator_amd import Engine, abi, framework as F, synth

NODES, PODS, BATCH = 300, 600, 16
XR_PODS = 32  # pods per exact round (kXrPods)
FIELDS = ("pods_scheduled", "pods_unschedulable", "device_batches", "node_evaluations", "reserved0", "reserved1")
_BASE = (F.NODE_RESOURCES_FIT, F.LOAD_AWARE)


def _cfg(*extra, **score):
    names = _BASE + extra
    prof = F.Profile(filter=names, score={**{k: 1 for k in names}, **score})
    return F.build_config(profile=prof, batch_pods=BATCH, pods_per_wave=8, pipeline_depth=1)


def _quotas(pods, seed, n_quotas=8):
    """limits of about a share of the queue's demand each, so some quotas run out (as tests/test_elasticquota.py)"""
    rng = np.random.default_rng(seed)
    pods["quota_id"] = np.where(rng.random(len(pods)) < 0.8, rng.integers(1, n_quotas + 1, len(pods)), 0)
    quotas = np.zeros(n_quotas, dtype=abi.QUOTA_DTYPE)
    share = pods["requests"][:, :2].sum(axis=0) // n_quotas
    quotas["used_limit"][:, 0] = (share[0] * rng.uniform(0.2, 1.2, n_quotas)).astype(np.int64)
    quotas["used_limit"][:, 1] = (share[1] * rng.uniform(0.2, 1.2, n_quotas)).astype(np.int64)
    quotas["min"][:, :2] = quotas["used_limit"][:, :2] // 4
    return quotas


def _fit_la(quota):
    cluster = synth.make_cluster(NODES, seed=synth.BASE_SEED + 300)
    pods = synth.make_pods(PODS, seed=synth.BASE_SEED + 301)
    quotas = _quotas(pods, synth.BASE_SEED + 302) if quota else None
    with Engine(_cfg(), cluster.n) as e:
        synth.load_into(e, cluster)
        if quota:
            e.set_quotas(quotas)
        return e.schedule(pods)[2]


def _numa():
    cluster, numa = synth.make_numa_cluster(NODES, seed=synth.BASE_SEED + 310)
    pods = synth.make_numa_pods(PODS, seed=synth.BASE_SEED + 311)
    with Engine(_cfg(F.NODE_NUMA_RESOURCE), cluster.n) as e:
        synth.load_numa_into(e, cluster, numa)
        return e.schedule(pods)[2]


def _deviceshare():
    cluster, dev = synth.make_gpu_cluster(NODES, seed=synth.BASE_SEED + 320)
    pods = synth.make_gpu_pods(PODS, seed=synth.BASE_SEED + 321)
    with Engine(_cfg(F.DEVICE_SHARE), cluster.n) as e:
        synth.load_gpu_into(e, cluster, dev)
        return e.schedule(pods)[2]


def _exact(n_pods):
    cluster, rsv = synth.make_rsv_cluster(NODES, seed=synth.BASE_SEED + 330)
    pods = synth.make_rsv_pods(PODS, seed=synth.BASE_SEED + 331)[:n_pods]
    with Engine(_cfg(F.RESERVATION, **{F.RESERVATION: 5000}), cluster.n) as e:
        synth.load_rsv_into(e, cluster, rsv)
        return e.schedule(pods)[2]


# case → (run, pods of the call, pods per round)
CASES = {
    "fit_la": (lambda: _fit_la(False), PODS, BATCH),
    "fit_la_quota": (lambda: _fit_la(True), PODS, BATCH),
    "numa": (_numa, PODS, BATCH),
    "deviceshare": (_deviceshare, PODS, BATCH),
    "exact": (lambda: _exact(PODS), PODS, XR_PODS),
    "exact_3": (lambda: _exact(3), 3, XR_PODS),
}


def record():
    """case → {field: value} for FIELDS, plus "active" = the resolvers' active time (reserved[2]) was counted"""
    out = {}
    for name, (run, _, _) in CASES.items():
        st = run()
        row = {k: int(st[k]) for k in FIELDS[:4]}
        row["reserved0"] = int(st["reserved"][0])
        row["reserved1"] = int(st["reserved"][1])
        row["active"] = bool(st["reserved"][2] > 0)
        out[name] = row
    return out
