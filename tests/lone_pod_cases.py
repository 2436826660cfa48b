"""The bad pods, profiles and entry points of tests/test_lone_pod_errors.py, shared with the recorder
tests/golden/make_lone_pod_errors.py: for every profile, entry point and case, (return code, kg_last_error() text).

Profiles (4-node tables):
  wide           NodeResourcesFit + LoadAware: no DeviceShare, so a device request is refused
  rsv            + Reservation, one reservation compiled against 8 predicates
  shipped        + NodeNUMAResource + DeviceShare, the same reservation
  shipped_rgpu   the same with the reservation holding a GPU (RDMA / FPGA pods and the dry run keep the Go path)
  defaults_rsv   Fit + LoadAware + TaintToleration + NodeAffinity + Reservation

Entry points: the eight single-pod ones, kg_pods_diagnose with the bad pod at batch index 0 and at 3."""
import numpy as np

from koordinator_amd import Engine, abi, framework as F, synth
from koordinator_amd.abi import KoordGPUError

N = 4
_BASE = (F.NODE_RESOURCES_FIT, F.LOAD_AWARE)


def _profile(*extra):
    names = _BASE + extra
    return F.Profile(filter=names, score={k: 1 for k in names})


PROFILES = {
    "wide": _profile(),
    "rsv": _profile(F.RESERVATION),
    "shipped": _profile(F.NODE_NUMA_RESOURCE, F.DEVICE_SHARE, F.RESERVATION),
    "shipped_rgpu": _profile(F.NODE_NUMA_RESOURCE, F.DEVICE_SHARE, F.RESERVATION),
    "defaults_rsv": _profile(F.TAINT_TOLERATION, F.NODE_AFFINITY, F.RESERVATION),
}


def _good():
    return F.make_pod({"cpu": "1", "memory": str(1 << 30)})


def _negative_cpu(p):
    p["requests"][0, abi.RES_CPU] = -5


def _device_request(p):
    p["device_requests"][0, abi.DEV_NVIDIA_GPU] = 1


def _rdma(p):
    p["device_requests"][0, abi.DEV_RDMA] = 100


def _reserve_pod(p):
    p["flags"][0] |= abi.POD_RESERVE


def _selector_above_table(p):
    p["reservation_flags"][0] |= abi.POD_RSV_AFFINITY
    p["reservation_selector"][0] = np.uint64(1) << np.uint64(40)  # the reservations know predicates 0..7


def _taint_count(p):
    p["flags"][0] |= abi.POD_TAINT_TABLE
    p["taint_count"][0] = 65


def _bad_qos(p):
    p["qos"][0] = 99


def _negative_device(p):
    p["device_requests"][0, abi.DEV_GPU_CORE] = -1


# name -> the faults applied to a good pod, in this order (the last four are wrong in two ways at once)
CASES = {
    "negative_cpu": (_negative_cpu,),
    "device_request": (_device_request,),
    "rdma": (_rdma,),
    "reserve_pod": (_reserve_pod,),
    "selector_above_table": (_selector_above_table,),
    "taint_count_65": (_taint_count,),
    "negative_cpu+device_request": (_negative_cpu, _device_request),
    "selector_above_table+taint_count_65": (_selector_above_table, _taint_count),
    "reserve_pod+bad_qos": (_reserve_pod, _bad_qos),
    "bad_qos+negative_device": (_bad_qos, _negative_device),
}


def make_case(name):
    p = _good()
    for fault in CASES[name]:
        fault(p)
    return p


def _reservations(gpu):
    rsv = np.zeros(N, dtype=abi.NODE_RSV_DTYPE)
    rsv["n"][0] = 1
    rsv["allocatable_cpu"][0, 0] = 4000
    rsv["allocatable_mem"][0, 0] = 8 << 30
    rsv["available"][0, 0] = 1
    rsv["predicate_count"] = 8
    if gpu:
        rsv["gpu_minors"][0, 0] = 1
        rsv["gpu_alloc"][0, 0, 0] = (100, synth.GPU_MEM, 100)
    return rsv


def open_engine(profile):
    cfg = F.build_config(profile=PROFILES[profile])
    e = Engine(cfg, N)
    if profile.startswith("shipped"):
        cluster, numa, dev, _ = synth.make_shipped_cluster(N, seed=7301)
        synth.load_shipped_into(e, cluster, numa, dev, _reservations(profile == "shipped_rgpu"))
    else:
        cluster = synth.make_cluster(N, seed=7302)
        synth.load_into(e, cluster)
        if profile != "wide":
            e.upsert_reservations(_reservations(False))
    return e, cluster


def _entry_points(e, cluster, pod):
    good = _good()
    nodes = np.arange(2, dtype=np.int32)
    vics = [cluster.existing_pods[cluster.existing_node == i][:2] for i in nodes]
    prios = [np.zeros(len(v), dtype=np.int32) for v in vics]
    starts = [np.zeros(len(v), dtype=np.int64) for v in vics]
    return {
        "evaluate_reservation": lambda: e.evaluate_reservation(pod),
        "debug_topn": lambda: e.debug_topn(pod, 2),
        "diagnose@0": lambda: e.diagnose(np.concatenate([pod, good, good, good])),
        "diagnose@3": lambda: e.diagnose(np.concatenate([good, good, good, pod])),
        "filter_preemption": lambda: e.filter_preemption(pod, 1, vics[1]),
        "select_victims": lambda: e.select_victims(pod, nodes, vics),
        "preempt": lambda: e.preempt(pod, nodes, vics, prios, starts),
        "evaluate_numa": lambda: e.evaluate_numa(pod),
        "evaluate_device": lambda: e.evaluate_device(pod),
    }


def record():
    """{profile: {entry point: {case: [code, text]}}}; an accepted pod is [0, ""]"""
    out = {}
    for profile in PROFILES:
        e, cluster = open_engine(profile)
        try:
            per = out.setdefault(profile, {})
            for case in CASES:
                for entry, call in _entry_points(e, cluster, make_case(case)).items():
                    try:
                        call()
                        got = [0, ""]
                    except KoordGPUError as ex:
                        got = [int(ex.code), str(ex)]
                    per.setdefault(entry, {})[case] = got
        finally:
            e.close()
    return out
