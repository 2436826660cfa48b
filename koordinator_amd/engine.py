"""Python handle over the koordgpu C ABI (the same entry points a cgo binding would call)."""
from __future__ import annotations

import ctypes

import numpy as np

from . import abi
from .abi import check, ptr


def default_config() -> np.ndarray:
    """kg_config_default: v1beta2 LoadAwareSchedulingArgs defaults + NodeResourcesFit LeastAllocated cpu/mem."""
    lib = abi.load_library()
    cfg = np.zeros(1, dtype=abi.CONFIG_DTYPE)
    lib.kg_config_default(ptr(cfg))
    return cfg


def nccl_unique_id() -> bytes:
    """ncclGetUniqueId on this rank (rank 0 creates it; the caller broadcasts the 128 bytes)."""
    lib = abi.load_library()
    buf = ctypes.create_string_buffer(128)
    check(lib, lib.kg_nccl_unique_id(ctypes.cast(buf, ctypes.c_void_p)))
    return buf.raw


class Loopback:
    """kg_loopback (test hook): n ranks' engines in one process exchanging their round records by device copies
    instead of RCCL.  Drive each rank's engine from its own thread (ctypes releases the GIL in the calls)."""

    def __init__(self, n_ranks: int):
        self.lib = abi.load_library()
        h = ctypes.c_void_p()
        check(self.lib, self.lib.kg_loopback_create(int(n_ranks), ctypes.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.kg_loopback_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class HostExchange:
    """kg_engine_create_hosted's exchange over a caller-side all-gather: `allgather(send: bytes-like uint8 array)`
    returns the n_ranks parts concatenated in rank order — e.g. torch.distributed.all_gather on gloo CPU tensors,
    so that several processes run the engine's multi-rank round path without RCCL."""

    def __init__(self, allgather):
        self.allgather = allgather
        self.error = None

        def _fn(user, send, recv, nbytes):
            try:
                buf = np.ctypeslib.as_array(ctypes.cast(send, ctypes.POINTER(ctypes.c_uint8)), shape=(int(nbytes),))
                out = np.ascontiguousarray(self.allgather(buf.copy()), dtype=np.uint8).reshape(-1)
                ctypes.memmove(recv, out.ctypes.data, out.nbytes)
                return 0
            except Exception as exc:  # reported through the engine's KG_E_COLLECTIVE
                self.error = exc
                return 1

        self.fn = abi.EXCHANGE_FN(_fn)  # kept alive as long as the engine


class Engine:
    """One engine = one rank's GPU-resident node table (replicated) + its evaluation shard."""

    def __init__(self, config: np.ndarray, capacity: int, rank: int = 0, n_ranks: int = 1,
                 nccl_id: bytes | None = None, loopback: Loopback | None = None,
                 exchange: HostExchange | None = None, fit_shape=None):
        self.lib = abi.load_library()
        self._cfg = np.array(config, dtype=abi.CONFIG_DTYPE).reshape(1)
        h = ctypes.c_void_p()
        idbuf = None
        if nccl_id is not None:
            idbuf = ctypes.create_string_buffer(bytes(nccl_id), 128)
        self._exchange = exchange
        if exchange is not None:
            check(self.lib, self.lib.kg_engine_create_hosted(ptr(self._cfg), int(capacity), int(rank), int(n_ranks),
                                                             exchange.fn, None, ctypes.byref(h)))
        elif loopback is not None:
            check(self.lib, self.lib.kg_engine_create_loopback(ptr(self._cfg), int(capacity), int(rank), int(n_ranks),
                                                               loopback.h, ctypes.byref(h)))
        else:
            check(self.lib, self.lib.kg_engine_create(ptr(self._cfg), int(capacity), int(rank), int(n_ranks),
                                                      ctypes.cast(idbuf, ctypes.c_void_p) if idbuf else None,
                                                      ctypes.byref(h)))
        self.h = h
        self.capacity = capacity
        if fit_shape is not None:  # NodeResourcesFit RequestedToCapacityRatio: kg_config cannot carry the shape
            try:
                self.set_fit_shape(fit_shape)
            except Exception:
                self.close()
                raise

    # -- lifecycle -------------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "h", None):
            self.lib.kg_engine_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- informer-style deltas ------------------------------------------------------------------------
    @staticmethod
    def _idx(idx, n):
        if idx is None:
            idx = np.arange(n, dtype=np.int32)
        return np.ascontiguousarray(idx, dtype=np.int32)

    def upsert_nodes(self, nodes: np.ndarray, idx=None):
        nodes = np.ascontiguousarray(nodes, dtype=abi.NODE_DTYPE)
        idx = self._idx(idx, len(nodes))
        check(self.lib, self.lib.kg_nodes_upsert(self.h, ptr(nodes), ptr(idx), len(nodes)))

    def delete_nodes(self, idx):
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        check(self.lib, self.lib.kg_nodes_delete(self.h, ptr(idx), len(idx)))

    def update_metrics(self, metrics: np.ndarray, now_ns: int, idx=None):
        metrics = np.ascontiguousarray(metrics, dtype=abi.METRIC_DTYPE)
        idx = self._idx(idx, len(metrics))
        check(self.lib, self.lib.kg_node_metrics_update(self.h, ptr(metrics), ptr(idx), len(metrics), int(now_ns)))

    def set_pods_metric(self, node: int, entries: np.ndarray):
        """kg_node_pods_metric_set: NodeMetric.Status.PodsMetric of one node (POD_METRIC_DTYPE rows)."""
        entries = np.ascontiguousarray(entries, dtype=abi.POD_METRIC_DTYPE)
        check(self.lib, self.lib.kg_node_pods_metric_set(self.h, int(node), ptr(entries) if len(entries) else None,
                                                          len(entries)))

    def add_pods(self, pods: np.ndarray, node_idx):
        pods = np.ascontiguousarray(pods, dtype=abi.POD_DTYPE)
        node_idx = np.ascontiguousarray(node_idx, dtype=np.int32)
        check(self.lib, self.lib.kg_pods_add(self.h, ptr(pods), ptr(node_idx), len(pods)))

    def remove_pods(self, pods: np.ndarray, node_idx):
        pods = np.ascontiguousarray(pods, dtype=abi.POD_DTYPE)
        node_idx = np.ascontiguousarray(node_idx, dtype=np.int32)
        check(self.lib, self.lib.kg_pods_remove(self.h, ptr(pods), ptr(node_idx), len(pods)))

    def unreserve(self, first: int, count: int, mask=None):
        """kg_pods_unreserve: the framework's Unreserve of staged pods [first, first+count) (mask selects them)."""
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        if m is not None and len(m) != count:
            raise ValueError("mask length != count")
        check(self.lib, self.lib.kg_pods_unreserve(self.h, int(first), int(count), ptr(m)))

    def set_clock(self, now_ns: int):
        """kg_engine_set_clock: > 0 fixed, 0 real time, < 0 the newest metrics update time."""
        check(self.lib, self.lib.kg_engine_set_clock(self.h, int(now_ns)))

    def upsert_numa(self, node_numa: np.ndarray, idx=None):
        """NodeNUMAResource state (TopologyOptions + NodeAllocation) of nodes `idx` (kg_nodes_numa_upsert)."""
        node_numa = np.ascontiguousarray(node_numa, dtype=abi.NODE_NUMA_DTYPE)
        idx = self._idx(idx, len(node_numa))
        check(self.lib, self.lib.kg_nodes_numa_upsert(self.h, ptr(node_numa), ptr(idx), len(node_numa)))

    def upsert_devices(self, node_device: np.ndarray, idx=None):
        """DeviceShare GPU state (Device object + deviceUsed) of nodes `idx` (kg_nodes_device_upsert)."""
        node_device = np.ascontiguousarray(node_device, dtype=abi.NODE_DEVICE_DTYPE)
        idx = self._idx(idx, len(node_device))
        check(self.lib, self.lib.kg_nodes_device_upsert(self.h, ptr(node_device), ptr(idx), len(node_device)))

    def upsert_reservations(self, node_rsv: np.ndarray, idx=None):
        """Reservation slots of nodes `idx` (kg_nodes_reservation_upsert)."""
        node_rsv = np.ascontiguousarray(node_rsv, dtype=abi.NODE_RSV_DTYPE)
        idx = self._idx(idx, len(node_rsv))
        check(self.lib, self.lib.kg_nodes_reservation_upsert(self.h, ptr(node_rsv), ptr(idx), len(node_rsv)))

    def upsert_predicates(self, preds: np.ndarray, idx=None):
        """TaintToleration / NodeAffinity node rows of nodes `idx` (kg_nodes_predicates_upsert; NODE_PRED_DTYPE, see
        koordinator_amd/predicates.py)."""
        preds = np.ascontiguousarray(preds, dtype=abi.NODE_PRED_DTYPE)
        idx = self._idx(idx, len(preds))
        check(self.lib, self.lib.kg_nodes_predicates_upsert(self.h, ptr(preds), ptr(idx), len(preds)))

    def read_reservations(self):
        """(allocated cpu, allocated memory, assigned), int64[n, KG_MAX_RSV_SLOTS] each, from the device."""
        n = self.num_nodes
        out = [np.zeros((n, abi.MAX_RSV_SLOTS), dtype=np.int64) for _ in range(3)]
        check(self.lib, self.lib.kg_nodes_read_reservations(self.h, *[ptr(o) for o in out]))
        return tuple(out)

    def read_reservation_gpus(self):
        """(ABI 13) the reservation slots' gpu_allocated, int64[n, KG_MAX_RSV_SLOTS, KG_MAX_MINORS, 3], from the device
        (kg_nodes_read_reservation_gpus)."""
        out = np.zeros((self.num_nodes, abi.MAX_RSV_SLOTS, abi.MAX_MINORS, 3), dtype=np.int64)
        check(self.lib, self.lib.kg_nodes_read_reservation_gpus(self.h, ptr(out)))
        return out

    def read_reservation_cpus(self):
        """(ABI 15) the reservation slots' cpus_assigned, uint64[n, KG_MAX_RSV_SLOTS, 4], from the device
        (kg_nodes_read_reservation_cpus)."""
        out = np.zeros((self.num_nodes, abi.MAX_RSV_SLOTS, abi.MAX_CPUS // 64), dtype=np.uint64)
        check(self.lib, self.lib.kg_nodes_read_reservation_cpus(self.h, ptr(out)))
        return out

    def read_pod_groups(self, zone: bool = False):
        """(ABI 12) per node and match group: (pods matching, required anti-affinity terms, symmetric weight) — and,
        with zone, the zone-keyed terms' (anti-affinity, symmetric weight) — int32[n, KG_MAX_MATCH_GROUPS] each, from
        the device (kg_nodes_read_pod_groups)."""
        n = self.num_nodes
        out = [np.zeros((n, abi.MAX_MATCH_GROUPS), dtype=np.int32) for _ in range(5)]
        check(self.lib, self.lib.kg_nodes_read_pod_groups(self.h, *[ptr(o) for o in out]))
        return tuple(out[:3]) if not zone else tuple(out)

    def fetch_reservations(self, first: int, count: int) -> np.ndarray:
        """int32[count]: the reservation slot Reserve assumed each staged pod into (-1 = none)."""
        out = np.zeros(count, dtype=np.int32)
        check(self.lib, self.lib.kg_results_fetch_reservations(self.h, int(first), int(count), ptr(out)))
        return out

    def set_quotas(self, quotas: np.ndarray):
        """ElasticQuota table (kg_quotas_set): pods' quota_id = 1 + index."""
        quotas = np.ascontiguousarray(quotas, dtype=abi.QUOTA_DTYPE)
        check(self.lib, self.lib.kg_quotas_set(self.h, ptr(quotas), len(quotas)))

    def read_quotas(self, n: int) -> np.ndarray:
        out = np.zeros(n, dtype=abi.QUOTA_DTYPE)
        check(self.lib, self.lib.kg_quotas_read(self.h, ptr(out), n))
        return out

    # -- hot path -----------------------------------------------------------------------------------------
    def schedule(self, pods: np.ndarray, priorities=None):
        """Sequential FIFO scheduling with assume; returns (node_idx[-1 = unschedulable], total_score, stats).
        priorities (PodPriority per pod): the call honours the nominated-pod table (schedule_staged_nominated)."""
        pods = np.ascontiguousarray(pods, dtype=abi.POD_DTYPE)
        n = len(pods)
        if priorities is not None:
            self.stage(pods)
            stats = self.schedule_staged(0, n, priorities)
            out_node, out_score = self.fetch(0, n)
            return out_node, out_score, stats
        out_node = np.empty(n, dtype=np.int32)
        out_score = np.empty(n, dtype=np.int64)
        stats = np.zeros(1, dtype=abi.STATS_DTYPE)
        check(self.lib, self.lib.kg_pods_schedule(self.h, ptr(pods), n, ptr(out_node), ptr(out_score), ptr(stats)))
        return out_node, out_score, stats[0]

    def stage(self, pods: np.ndarray):
        pods = np.ascontiguousarray(pods, dtype=abi.POD_DTYPE)
        check(self.lib, self.lib.kg_pods_stage(self.h, ptr(pods), len(pods)))

    def schedule_staged(self, first: int, count: int, priorities=None):
        """kg_pods_schedule_staged; with priorities (PodPriority of staged pods first .. first + count)
        kg_pods_schedule_staged_nominated, which honours the nominated-pod table."""
        stats = np.zeros(1, dtype=abi.STATS_DTYPE)
        if priorities is None:
            check(self.lib, self.lib.kg_pods_schedule_staged(self.h, int(first), int(count), ptr(stats)))
            return stats[0]
        pr = np.ascontiguousarray(priorities, dtype=np.int32)
        if len(pr) != count:
            raise ValueError(f"{len(pr)} priorities for {count} pods")
        check(self.lib, self.lib.kg_pods_schedule_staged_nominated(self.h, int(first), int(count), ptr(pr), ptr(stats)))
        return stats[0]

    # -- nominated pods -----------------------------------------------------------------------------------
    def set_nominated(self, pods, node_idx, priorities):
        """kg_nominated_pods_set: REPLACES the nominated-pod table (empty arrays empty it)."""
        pods = np.ascontiguousarray(pods, dtype=abi.POD_DTYPE).reshape(-1)
        nodes = np.ascontiguousarray(node_idx, dtype=np.int32).reshape(-1)
        pr = np.ascontiguousarray(priorities, dtype=np.int32).reshape(-1)
        if not (len(pods) == len(nodes) == len(pr)):
            raise ValueError("set_nominated: pods, node_idx and priorities differ in length")
        check(self.lib, self.lib.kg_nominated_pods_set(self.h, len(pods), ptr(pods), ptr(nodes), ptr(pr)))

    def read_nominated(self):
        """kg_nominated_pods_read: the live entries of the DEVICE copy in stored order — (node, priority descending) —
        as (uid int64[n], node int32[n], priority int32[n])."""
        n = np.zeros(1, np.int64)
        cap = abi.MAX_NOMINATED
        uid, node, pr = np.zeros(cap, np.int64), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        check(self.lib, self.lib.kg_nominated_pods_read(self.h, cap, ptr(uid), ptr(node), ptr(pr), ptr(n)))
        k = int(n[0])
        return uid[:k].copy(), node[:k].copy(), pr[:k].copy()

    def filter_nominated(self, pod: np.ndarray, priority: int):
        """kg_pods_filter_nominated: per node (reject bits of the pass with the nominated pods added, entries added)."""
        pod = np.ascontiguousarray(np.asarray(pod, dtype=abi.POD_DTYPE).reshape(1))
        n = self.num_nodes
        rej, added = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
        check(self.lib, self.lib.kg_pods_filter_nominated(self.h, ptr(pod), int(priority), ptr(rej), ptr(added)))
        return rej[:n], added[:n]

    def nominated_counters(self) -> dict:
        """kg_nominated_counters since the last set_nominated: pods through the unchanged paths, pods through the
        per-pod pass with the table, entries removed by placement."""
        out = np.zeros(3, np.int64)
        check(self.lib, self.lib.kg_nominated_counters(self.h, ptr(out)))
        return {"plain": int(out[0]), "nominated": int(out[1]), "removed": int(out[2])}

    def fetch(self, first: int, count: int):
        out_node = np.empty(count, dtype=np.int32)
        out_score = np.empty(count, dtype=np.int64)
        check(self.lib, self.lib.kg_results_fetch(self.h, int(first), int(count), ptr(out_node), ptr(out_score)))
        return out_node, out_score

    def evaluate(self, pod: np.ndarray):
        """Per-node reject bits, NodeResourcesFit score, LoadAwareScheduling score for one pod (no assume)."""
        pod = np.ascontiguousarray(np.asarray(pod, dtype=abi.POD_DTYPE).reshape(1))
        n = self.num_nodes
        rej = np.zeros(n, dtype=np.int32)
        fit = np.zeros(n, dtype=np.int64)
        la = np.zeros(n, dtype=np.int64)
        check(self.lib, self.lib.kg_pods_evaluate(self.h, ptr(pod), ptr(rej), ptr(fit), ptr(la)))
        return rej, fit, la

    def evaluate_numa(self, pod: np.ndarray):
        """NodeNUMAResource alone on every node: (passes Filter, Score, stored affinity mask or -1 for nil)."""
        pod = np.ascontiguousarray(np.asarray(pod, dtype=abi.POD_DTYPE).reshape(1))
        n = self.num_nodes
        ok = np.zeros(n, dtype=np.int32)
        sc = np.zeros(n, dtype=np.int64)
        af = np.zeros(n, dtype=np.int64)
        check(self.lib, self.lib.kg_pods_evaluate_numa(self.h, ptr(pod), ptr(ok), ptr(sc), ptr(af)))
        return ok, sc, af

    def evaluate_device(self, pod: np.ndarray):
        """DeviceShare alone on every node: (passes Filter, raw Score before NormalizeScore)."""
        pod = np.ascontiguousarray(np.asarray(pod, dtype=abi.POD_DTYPE).reshape(1))
        n = self.num_nodes
        ok = np.zeros(n, dtype=np.int32)
        sc = np.zeros(n, dtype=np.int64)
        check(self.lib, self.lib.kg_pods_evaluate_device(self.h, ptr(pod), ptr(ok), ptr(sc)))
        return ok, sc

    def fetch_devices(self, first: int, count: int) -> np.ndarray:
        """int32[count]: the GPU minor bitmask DeviceShare Reserve allocated to each staged pod (0 = none)."""
        out = np.zeros(count, dtype=np.int32)
        check(self.lib, self.lib.kg_results_fetch_devices(self.h, int(first), int(count), ptr(out)))
        return out

    def fetch_devices_x(self, first: int, count: int) -> np.ndarray:
        """int32[count, 2]: the RDMA / FPGA minor bitmasks DeviceShare Reserve allocated to each staged pod (ABI 17)."""
        out = np.zeros((count, abi.DEV_XTYPES), dtype=np.int32)
        check(self.lib, self.lib.kg_results_fetch_devices_x(self.h, int(first), int(count), ptr(out)))
        return out

    def read_devices_x(self) -> np.ndarray:
        """int64[n, 2, 8]: the RDMA / FPGA deviceUsed from the device (ABI 17)."""
        out = np.zeros((self.num_nodes, abi.DEV_XTYPES, abi.MAX_MINORS), dtype=np.int64)
        check(self.lib, self.lib.kg_nodes_read_device_x(self.h, ptr(out)))
        return out

    def read_devices(self):
        """(used core, used memory, used ratio), int64[n, 8] each, from the device."""
        n = self.num_nodes
        out = [np.zeros((n, abi.MAX_MINORS), dtype=np.int64) for _ in range(3)]
        check(self.lib, self.lib.kg_nodes_read_device(self.h, *[ptr(o) for o in out]))
        return tuple(out)

    def fetch_cpusets(self, first: int, count: int) -> np.ndarray:
        """uint64[count, 4]: the cpuset NodeNUMAResource Reserve allocated to each staged pod (empty = none)."""
        out = np.zeros((count, abi.MAX_CPUS // 64), dtype=np.uint64)
        check(self.lib, self.lib.kg_results_fetch_cpusets(self.h, int(first), int(count), ptr(out)))
        return out

    # -- introspection -----------------------------------------------------------------------------------
    @property
    def ranks(self) -> tuple:
        """(ABI 15) (ranks node evaluation is sharded over, ranks this engine replicates) — kg_engine_ranks."""
        s, r = ctypes.c_int64(), ctypes.c_int64()
        check(self.lib, self.lib.kg_engine_ranks(self.h, ctypes.byref(s), ctypes.byref(r)))
        return int(s.value), int(r.value)

    @property
    def num_nodes(self) -> int:
        return int(self.lib.kg_engine_num_nodes(self.h))

    def read_state(self) -> dict:
        n = self.num_nodes
        names = ("requested_cpu", "requested_mem", "nonzero_cpu", "nonzero_mem", "num_pods",
                 "la_est_cpu", "la_est_mem", "la_est_prod_cpu", "la_est_prod_mem")
        out = {k: np.zeros(n, dtype=np.int64) for k in names}
        check(self.lib, self.lib.kg_nodes_read_state(self.h, *[ptr(out[k]) for k in names]))
        return out

    def read_numa(self):
        """(allocated cpus uint64[n,4], per-NUMA allocated cpu int64[n,4], memory int64[n,4]) from the device."""
        n = self.num_nodes
        alloc = np.zeros((n, abi.MAX_CPUS // 64), dtype=np.uint64)
        cpu = np.zeros((n, abi.MAX_NUMA), dtype=np.int64)
        mem = np.zeros((n, abi.MAX_NUMA), dtype=np.int64)
        check(self.lib, self.lib.kg_nodes_read_numa(self.h, ptr(alloc), ptr(cpu), ptr(mem)))
        return alloc, cpu, mem

    def bench_kernel(self, which: int, iters: int):
        ms = ctypes.c_double()
        by = ctypes.c_double()
        check(self.lib, self.lib.kg_bench_kernel(self.h, int(which), int(iters), ctypes.byref(ms), ctypes.byref(by)))
        return ms.value, by.value

    def profile(self, on: bool = True):
        """Live kernel timing of the round runners (kg_profile_enable): resets the accumulators."""
        check(self.lib, self.lib.kg_profile_enable(self.h, int(on)))

    def profile_read(self) -> dict:
        """{kernel name: (summed event ms, launches)} since profile() (kg_profile_read)."""
        ms = np.zeros(abi.PROF_KINDS, dtype=np.float64)
        n = np.zeros(abi.PROF_KINDS, dtype=np.int64)
        check(self.lib, self.lib.kg_profile_read(self.h, ptr(ms), ptr(n)))
        return {name: (float(ms[k]), int(n[k])) for k, name in abi.PROF_NAMES.items() if n[k] > 0}

    def debug_eval_paths(self) -> int:
        out = np.zeros(1, dtype=np.int64)
        check(self.lib, self.lib.kg_debug_eval_paths(self.h, ptr(out)))
        return int(out[0])

    def debug_round_records(self, first: int, nb: int):
        """One round's wide pass and local merge over the staged pods [first, first + nb), read back
        (kg_debug_round_records; a test hook, the table is left as it was).  Returns (geom, lists, records): geom a dict
        over abi.DBG_GEOM_FIELDS, lists uint64[nb, n_lists, list_len], records uint64[nb, kc + 1] (keys, then ub)."""
        geom = np.zeros(abi.DBG_GEOM_WORDS, dtype=np.int64)
        probe = np.zeros(1, dtype=np.uint64)
        # sizing call: the geometry is written before the (empty) lists buffer is refused
        rc = self.lib.kg_debug_round_records(self.h, int(first), int(nb), ptr(geom), ptr(probe), 0, ptr(probe))
        g = dict(zip(abi.DBG_GEOM_FIELDS, (int(x) for x in geom)))
        if rc == 0 or g["n_lists"] <= 0:
            check(self.lib, rc)
            raise RuntimeError("kg_debug_round_records accepted an empty lists buffer")
        lists = np.zeros((int(nb), g["n_lists"], g["list_len"]), dtype=np.uint64)
        records = np.zeros((int(nb), g["kc"] + 1), dtype=np.uint64)
        check(self.lib, self.lib.kg_debug_round_records(self.h, int(first), int(nb), ptr(geom), ptr(lists), lists.size,
                                                        ptr(records)))
        return g, lists, records

    def debug_merge(self, variant: int, lists: np.ndarray, kc: int = 64) -> np.ndarray:
        """The merge kernels on caller-given lists uint64[n_pods, n_lists, list_len] (kg_debug_merge; a test hook):
        variant 0 the per-wavefront merge, 1 the per-block merge of tile lists, 2 the per-block merge of rank records.
        Returns the records uint64[n_pods, kc + 1] (keys, then ub)."""
        lists = np.ascontiguousarray(lists, dtype=np.uint64)
        if lists.ndim != 3:
            raise ValueError("lists: uint64[n_pods, n_lists, list_len]")
        n_pods, n_lists, list_len = lists.shape
        out = np.zeros((n_pods, kc + 1), dtype=np.uint64)
        check(self.lib, self.lib.kg_debug_merge(self.h, int(variant), ptr(lists), n_pods, n_lists, list_len, ptr(out)))
        return out

    def debug_resolve(self, first: int, nb: int, prev=(), poison: bool = False, cursor=None):
        """The product's resolver on a staged situation (kg_debug_resolve; a test hook): eval + merge of the staged pods
        [first, first + nb) on the table as it stands, then the earlier rounds `prev` — a sequence of lists of
        (staged pod index, node) pairs, prev[0] the round just before this one — applied to the table and to the
        modified-row lists, then the resolver.  poison / cursor: a stale round.  Returns a dict: the control words and
        constants over abi.DBG_RESOLVE_FIELDS, 'records' uint64[nb, kc + 1], 'out_keys' uint64[nb], 'list' int32[n]."""
        counts = np.array([len(l) for l in prev], dtype=np.int64)
        pairs = np.array([pr for l in prev for pr in l], dtype=np.int32).reshape(-1, 2)
        pods = np.ascontiguousarray(pairs[:, 0])
        nodes = np.ascontiguousarray(pairs[:, 1])
        flags = (abi.DBG_RESOLVE_POISON if poison else 0) | (abi.DBG_RESOLVE_CURSOR if cursor is not None else 0)
        info = np.zeros(abi.DBG_RESOLVE_WORDS, dtype=np.int64)
        records = np.zeros((int(nb), 65), dtype=np.uint64)  # kC + 1 words per pod; checked against info below
        keys = np.zeros(int(nb), dtype=np.uint64)
        lst = np.zeros(64, dtype=np.int32)
        check(self.lib, self.lib.kg_debug_resolve(self.h, int(first), int(nb), len(counts), ptr(counts), ptr(pods),
                                                  ptr(nodes), flags, int(cursor or 0), ptr(info), ptr(records),
                                                  ptr(keys), ptr(lst)))
        out = dict(zip(abi.DBG_RESOLVE_FIELDS, (int(x) for x in info)))
        if out["kc"] + 1 != records.shape[1]:
            raise RuntimeError(f"kg_debug_resolve: records of {out['kc']} keys, the binding sized them for 64")
        out.update(records=records, out_keys=keys, list=lst[:out["n_list"]].copy())
        return out

    def filter_preemption(self, pod: np.ndarray, node: int, victims: np.ndarray, slots=None, minors=None) -> int:
        """The preemption dry run's Filter of `pod` on node `node` with `victims` removed (kg_pods_filter_preemption):
        KG_REJECT_* bits, 0 = fits.  slots[k]: the node's reservation slot victim k was allocated from (-1 = none);
        minors[k]: the GPU minors (bitmask) its DeviceShare allocation holds on the node (0 = none)."""
        pod = np.ascontiguousarray(np.asarray(pod, dtype=abi.POD_DTYPE).reshape(1))
        victims = np.ascontiguousarray(np.asarray(victims, dtype=abi.POD_DTYPE).reshape(-1))
        sl = None if slots is None else np.ascontiguousarray(slots, dtype=np.int32)
        mi = None if minors is None else np.ascontiguousarray(minors, dtype=np.int32)
        out = np.zeros(1, dtype=np.int32)
        check(self.lib, self.lib.kg_pods_filter_preemption(self.h, ptr(pod), int(node), ptr(victims) if len(victims) else None,
                                                           ptr(sl) if sl is not None else None,
                                                           ptr(mi) if mi is not None else None, len(victims), ptr(out)))
        return int(out[0])

    def select_victims(self, pod: np.ndarray, nodes, victims_per_node, slots_per_node=None, violating_per_node=None,
                       minors_per_node=None):
        """SelectVictimsOnNode on every candidate node in one launch (kg_pods_select_victims).  victims_per_node[c]:
        candidate c's potential victims (POD_DTYPE) in reprieve order; slots / violating / minors: per-victim reservation
        slot (-1 none), PDB-violating flag and GPU minors.  Returns (reject int32[C], victim bool arrays per candidate,
        violating int32[C])."""
        pod = np.ascontiguousarray(np.asarray(pod, dtype=abi.POD_DTYPE).reshape(1))
        nodes = np.ascontiguousarray(nodes, dtype=np.int32)
        counts = np.array([len(v) for v in victims_per_node], dtype=np.int64)
        off = np.zeros(len(nodes) + 1, dtype=np.int64)
        off[1:] = np.cumsum(counts)
        nv = int(off[-1])
        vic = np.zeros(max(nv, 1), dtype=abi.POD_DTYPE)
        if nv:
            vic[:nv] = np.concatenate([np.asarray(v, dtype=abi.POD_DTYPE).reshape(-1) for v in victims_per_node])
        sl = vio = mi = None
        if minors_per_node is not None and nv:
            mi = np.ascontiguousarray(np.concatenate([np.asarray(s, dtype=np.int32).reshape(-1)
                                                      for s in minors_per_node]))
        if slots_per_node is not None and nv:
            sl = np.ascontiguousarray(np.concatenate([np.asarray(s, dtype=np.int32).reshape(-1)
                                                      for s in slots_per_node]))
        if violating_per_node is not None and nv:
            vio = np.ascontiguousarray(np.concatenate([np.asarray(s, dtype=np.uint8).reshape(-1)
                                                       for s in violating_per_node]))
        rej = np.zeros(max(len(nodes), 1), dtype=np.int32)
        kept = np.zeros(max(nv, 1), dtype=np.uint8)
        nvio = np.zeros(max(len(nodes), 1), dtype=np.int32)
        check(self.lib, self.lib.kg_pods_select_victims(self.h, ptr(pod), len(nodes), ptr(nodes), ptr(off), ptr(vic),
                                                        ptr(sl) if sl is not None else None,
                                                        ptr(mi) if mi is not None else None,
                                                        ptr(vio) if vio is not None else None, ptr(rej), ptr(kept),
                                                        ptr(nvio)))
        return (rej[:len(nodes)], [kept[off[c]:off[c + 1]].astype(bool) for c in range(len(nodes))],
                nvio[:len(nodes)])

    def pick_candidate(self, nodes, victim_offsets, reject, kept, num_violating, victim_priority, victim_start,
                       victims_cap: int | None = None):
        """(added within ABI 18) kg_pods_pick_candidate: upstream's SelectCandidate / pickOneNodeForPreemption reduced
        on the device, over per-candidate dry-run results the caller holds (what select_victims returned, possibly
        edited by extenders).  victim_offsets: int64[C + 1] into the flat per-victim arrays `kept` (uint8),
        `victim_priority` (int32) and `victim_start` (int64 unix nanoseconds); reject / num_violating: int32[C].
        Returns (pick, victims): one abi.PREEMPT_PICK_DTYPE record (candidate = -1: no eligible candidate) and the
        winner's victims as int32 positions into the flat arrays, in list order.  victims_cap: the room for them
        (default: the longest segment; smaller is refused).  The engine's state is unchanged."""
        nodes = np.ascontiguousarray(nodes, dtype=np.int32)
        off = np.ascontiguousarray(victim_offsets, dtype=np.int64)
        nc = len(nodes)
        if len(off) != nc + 1:
            raise ValueError("victim_offsets: one entry per candidate and the total")
        rej = np.ascontiguousarray(reject, dtype=np.int32)
        nvio = np.ascontiguousarray(num_violating, dtype=np.int32)
        kp = np.ascontiguousarray(kept, dtype=np.uint8)
        pr = np.ascontiguousarray(victim_priority, dtype=np.int32)
        stt = np.ascontiguousarray(victim_start, dtype=np.int64)
        nv = int(off[-1])
        if len(rej) < nc or len(nvio) < nc or min(len(kp), len(pr), len(stt)) < nv:
            raise ValueError("pick_candidate: an array is shorter than the candidates / victims it describes")
        cap = int(np.diff(off).max(initial=0)) if victims_cap is None else int(victims_cap)
        pick = np.zeros(1, dtype=abi.PREEMPT_PICK_DTYPE)
        out = np.zeros(max(cap, 1), dtype=np.int32)
        check(self.lib, self.lib.kg_pods_pick_candidate(self.h, nc, ptr(nodes), ptr(off), ptr(rej), ptr(kp), ptr(nvio),
                                                        ptr(pr), ptr(stt), ptr(pick), ptr(out), cap))
        return pick[0], out[:int(pick[0]["n_victims"])]

    def preempt(self, pod: np.ndarray, nodes, victims_per_node, priorities_per_node, starts_per_node,
                slots_per_node=None, violating_per_node=None, minors_per_node=None, want_reject: bool = False,
                victims_cap: int | None = None):
        """(added within ABI 18) kg_pods_preempt: the dry run of select_victims and SelectCandidate's pick in one call;
        only the pick comes back.  victims_per_node / slots / violating / minors as for select_victims;
        priorities_per_node[c] (int32) and starts_per_node[c] (int64 unix nanoseconds): PodPriority and the start time
        of candidate c's potential victims.  Returns (pick, victims): one abi.PREEMPT_PICK_DTYPE record (candidate =
        -1: nobody can make room) and the winner's victims as indices into victims_per_node[pick["candidate"]], in list
        order; with want_reject also the int32[C] per-candidate status words.  The engine's state is unchanged."""
        pod = np.ascontiguousarray(np.asarray(pod, dtype=abi.POD_DTYPE).reshape(1))
        nodes = np.ascontiguousarray(nodes, dtype=np.int32)
        nc = len(nodes)
        off = np.zeros(nc + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(v) for v in victims_per_node], dtype=np.int64)
        nv = int(off[-1])

        def flat(per_node, dtype):
            if not nv:
                return np.zeros(1, dtype=dtype)
            # joined as bytes: numpy concatenates records field by field, ten times slower at 100k lists
            parts = [np.ascontiguousarray(np.asarray(v, dtype=dtype).reshape(-1)).view(np.uint8) for v in per_node]
            a = np.concatenate(parts).view(dtype)
            if len(a) != nv:
                raise ValueError("preempt: a per-victim list does not match its node's victims")
            return a

        vic = flat(victims_per_node, abi.POD_DTYPE)
        pr = flat(priorities_per_node, np.int32)
        stt = flat(starts_per_node, np.int64)
        sl = flat(slots_per_node, np.int32) if slots_per_node is not None and nv else None
        vio = flat(violating_per_node, np.uint8) if violating_per_node is not None and nv else None
        mi = flat(minors_per_node, np.int32) if minors_per_node is not None and nv else None
        cap = int(np.diff(off).max(initial=0)) if victims_cap is None else int(victims_cap)
        pick = np.zeros(1, dtype=abi.PREEMPT_PICK_DTYPE)
        out = np.zeros(max(cap, 1), dtype=np.int32)
        rej = np.zeros(max(nc, 1), dtype=np.int32) if want_reject else None
        check(self.lib, self.lib.kg_pods_preempt(self.h, ptr(pod), nc, ptr(nodes), ptr(off), ptr(vic), ptr(sl), ptr(mi),
                                                 ptr(vio), ptr(pr), ptr(stt), ptr(pick), ptr(out), cap, ptr(rej)))
        c = int(pick[0]["candidate"])
        victims = out[:int(pick[0]["n_victims"])] - (off[c] if c >= 0 else 0)
        victims = victims.astype(np.int32)
        return (pick[0], victims, rej[:nc]) if want_reject else (pick[0], victims)

    # -- the resident bound-pod table (added within ABI 18) ------------------------------------------------
    def set_bound_pods(self, nodes, pods_per_node, priorities_per_node, starts_per_node, slots_per_node=None,
                       minors_per_node=None, pdb_masks_per_node=None):
        """kg_node_bound_pods_set: replaces the bound-pod list (NodeInfo.Pods) of each node of `nodes`; an empty list
        clears it.  pods_per_node[l]: POD_DTYPE records; priorities (PodPriority), starts (GetPodStartTime, unix
        nanoseconds), slots / minors (as for select_victims) and pdb_masks (uint64, bit b = the pod matches PDB b and is
        not in its DisruptedPods) per pod.  A priority outside int32 is refused with E_INVALID."""
        nodes = np.ascontiguousarray(nodes, dtype=np.int32)
        off = np.zeros(len(nodes) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(v) for v in pods_per_node], dtype=np.int64)
        nv = int(off[-1])

        def flat(per_node, dtype):
            if not nv:
                return np.zeros(1, dtype=dtype)
            # joined as bytes: numpy concatenates records field by field, ten times slower at 100k lists
            parts = [np.ascontiguousarray(np.asarray(v, dtype=dtype).reshape(-1)).view(np.uint8) for v in per_node]
            a = np.concatenate(parts).view(dtype)
            if len(a) != nv:
                raise ValueError("set_bound_pods: a per-pod list does not match its node's pods")
            return a

        pr64 = flat(priorities_per_node, np.int64)
        if nv and (pr64.min() < -2**31 or pr64.max() > 2**31 - 1):
            raise abi.KoordGPUError(abi.E_INVALID, "set_bound_pods: a priority outside int32")
        pods = flat(pods_per_node, abi.POD_DTYPE)
        pr = pr64.astype(np.int32)
        stt = flat(starts_per_node, np.int64)
        sl = flat(slots_per_node, np.int32) if slots_per_node is not None and nv else None
        mi = flat(minors_per_node, np.int32) if minors_per_node is not None and nv else None
        pm = flat(pdb_masks_per_node, np.uint64) if pdb_masks_per_node is not None and nv else None
        check(self.lib, self.lib.kg_node_bound_pods_set(self.h, len(nodes), ptr(nodes), ptr(off), ptr(pods), ptr(pr),
                                                        ptr(stt), ptr(sl), ptr(mi), ptr(pm)))

    def read_bound_pods(self, node: int):
        """kg_nodes_read_bound_pods: node's list from the DEVICE copy in stored (MoreImportantPod) order.  Returns (uid
        int64[len], caller-list index int32[len], info) with info = {"live": entries of all lists, "used": slab entries
        in use, "relocations", "compactions"}."""
        n, live, counters = np.zeros(1, np.int64), np.zeros(1, np.int64), np.zeros(3, np.int64)
        check(self.lib, self.lib.kg_nodes_read_bound_pods(self.h, int(node), None, None, 0, ptr(n), ptr(live), None))
        cap = int(n[0])
        uid, idx = np.zeros(max(cap, 1), np.int64), np.zeros(max(cap, 1), np.int32)
        check(self.lib, self.lib.kg_nodes_read_bound_pods(self.h, int(node), ptr(uid), ptr(idx), cap, ptr(n), ptr(live),
                                                          ptr(counters)))
        info = {"live": int(live[0]), "used": int(counters[0]), "relocations": int(counters[1]),
                "compactions": int(counters[2])}
        return uid[:cap], idx[:cap], info

    def _resident_args(self, pod, nodes, pdb_allowed):
        pod = np.ascontiguousarray(np.asarray(pod, dtype=abi.POD_DTYPE).reshape(1))
        nodes = None if nodes is None else np.ascontiguousarray(nodes, dtype=np.int32)
        nc = self.num_nodes if nodes is None else len(nodes)
        pdb = np.ascontiguousarray(pdb_allowed if pdb_allowed is not None else [], dtype=np.int32)
        return pod, nodes, nc, pdb

    def select_victims_resident(self, pod: np.ndarray, priority: int, pdb_allowed=None, nodes=None,
                                quota_rule: bool = True, entries: int | None = None):
        """kg_pods_select_victims_resident: SelectVictimsOnNode over the resident table, unfused.  nodes = None: every
        node slot.  entries: the candidates' resident entries (room of the per-entry outputs; default: the table's live
        count, enough for candidates named once).  Returns (reject int32[C], violating int32[C], potential int32[C],
        entry flags uint8[E], entry rank int32[E]): the per-entry arrays in candidate order, then the caller's list
        order; flags = abi.ENTRY_POTENTIAL | ENTRY_VIOLATING | ENTRY_VICTIM, rank = the place in reprieve order or -1."""
        pod, nodes, nc, pdb = self._resident_args(pod, nodes, pdb_allowed)
        if entries is None:
            entries = self.read_bound_pods(0)[2]["live"] if self.num_nodes else 0
        rej, nvio, npot = (np.zeros(max(nc, 1), dtype=np.int32) for _ in range(3))
        ef, er = np.zeros(max(entries, 1), dtype=np.uint8), np.full(max(entries, 1), -1, dtype=np.int32)
        check(self.lib, self.lib.kg_pods_select_victims_resident(
            self.h, ptr(pod), int(priority), abi.PREEMPT_RULE_QUOTA if quota_rule else 0, nc, ptr(nodes), ptr(pdb),
            len(pdb), ptr(rej), ptr(nvio), ptr(npot), ptr(ef), ptr(er), int(entries)))
        return rej[:nc], nvio[:nc], npot[:nc], ef[:entries], er[:entries]

    def preempt_resident(self, pod: np.ndarray, priority: int, pdb_allowed=None, nodes=None, quota_rule: bool = True,
                         want_reject: bool = False, victims_cap: int = 1024):
        """kg_pods_preempt_resident: the dry run over the resident table and SelectCandidate's pick in one call.
        Returns (pick, victim uids int64[n_victims], victim caller-list indices int32[n_victims]) in Victims.Pods order,
        with want_reject also the int32[C] status words.  victims_cap: the room for the winner's victims; below the
        longest resident list among the candidates it is refused.  The engine's state is unchanged."""
        pod, nodes, nc, pdb = self._resident_args(pod, nodes, pdb_allowed)
        pick = np.zeros(1, dtype=abi.PREEMPT_PICK_DTYPE)
        uid, idx = np.zeros(max(victims_cap, 1), np.int64), np.zeros(max(victims_cap, 1), np.int32)
        rej = np.zeros(max(nc, 1), dtype=np.int32) if want_reject else None
        check(self.lib, self.lib.kg_pods_preempt_resident(
            self.h, ptr(pod), int(priority), abi.PREEMPT_RULE_QUOTA if quota_rule else 0, nc, ptr(nodes), ptr(pdb),
            len(pdb), ptr(pick), ptr(uid), ptr(idx), int(victims_cap), ptr(rej)))
        nv = int(pick[0]["n_victims"])
        out = (pick[0], uid[:nv].copy(), idx[:nv].copy())
        return out + (rej[:nc],) if want_reject else out

    def evaluate_reservation(self, pod: np.ndarray) -> dict:
        """The exact pass's evaluation of one pod on every node (kg_pods_evaluate_reservation): per node pass,
        nominated slot, raw Reservation score, restore state (has_state, matched slots, restored Requested /
        NonZeroRequested / pod count, podRequested), the non-normalized weighted total and the raw DeviceShare score."""
        pod = np.ascontiguousarray(np.asarray(pod, dtype=abi.POD_DTYPE).reshape(1))
        n = self.num_nodes
        out = np.zeros((max(n, 1), abi.RSV_EVAL_WORDS), dtype=np.int64)
        check(self.lib, self.lib.kg_pods_evaluate_reservation(self.h, ptr(pod), ptr(out)))
        out = out[:n]
        names = ("pass", "nominated", "score", "has_state", "matched", "requested_cpu", "requested_mem", "nonzero_cpu",
                 "nonzero_mem", "num_pods", "pod_requested_cpu", "pod_requested_mem", "base", "ds_raw", "order")
        return {k: out[:, q] for q, k in enumerate(names)}

    def debug_topn(self, pod: np.ndarray, topn: int, out: np.ndarray | None = None):
        """(ABI 18) kg_debug_topn: the --debug-scores table of one pod, ranked on the device.  Returns (rows, feasible):
        rows = the min(topn, feasible) best feasible nodes as abi.TOPN_ROW_DTYPE (total descending, ties on the lowest
        node index; plugin[abi.PL_*] = each plugin's weighted, normalised Score, -1 = not enabled at Score), feasible =
        the number of feasible nodes.  Nothing is assumed: the engine's state is unchanged.  `out`: a caller-owned
        TOPN_ROW_DTYPE array of at least `topn` rows to fill (rows past the returned ones are left untouched)."""
        pod = np.ascontiguousarray(np.asarray(pod, dtype=abi.POD_DTYPE).reshape(1))
        if out is None:
            out = np.zeros(max(int(topn), 1), dtype=abi.TOPN_ROW_DTYPE)
        elif out.dtype != abi.TOPN_ROW_DTYPE or not out.flags["C_CONTIGUOUS"] or len(out) < int(topn):
            raise ValueError("out: a C-contiguous TOPN_ROW_DTYPE array of at least topn rows")
        counts = np.zeros(2, dtype=np.int64)
        check(self.lib, self.lib.kg_debug_topn(self.h, ptr(pod), int(topn), ptr(out), ptr(counts[0:1]), ptr(counts[1:2])))
        return out[:int(counts[0])], int(counts[1])

    def diagnose(self, pods: np.ndarray, node_status: bool = False):
        """(added within ABI 18) kg_pods_diagnose: framework.FitError of `pods`, reduced on the device.  Returns an
        abi.FIT_DIAG_DTYPE array, one record per pod: num_all_nodes, feasible, plugin_nodes[abi.PL_*] (the nodes whose
        status comes from that plugin: the first Filter that failed, in the profile's Filter order) and
        reason_nodes[b] (the nodes whose status carries abi.REJECT_* bit b).  Every pod is evaluated as the next pod
        against the same current state; nothing is assumed and the engine's state is unchanged.  With node_status also
        the (len(pods), num_nodes) int32 matrix of the per-node words (0 = feasible, abi.REJECT_INVALID_NODE alone = an
        invalid slot): the NodeToStatusMap a PostFilter receives, and the only n-sized copy."""
        pods = np.ascontiguousarray(np.asarray(pods, dtype=abi.POD_DTYPE).reshape(-1))
        n = len(pods)
        out = np.zeros(max(n, 1), dtype=abi.FIT_DIAG_DTYPE)
        status = np.zeros((n, self.num_nodes), dtype=np.int32) if node_status else None
        check(self.lib, self.lib.kg_pods_diagnose(self.h, ptr(pods) if n else None, n, ptr(out),
                                                  ptr(status) if node_status and status.size else None))
        return (out[:n], status) if node_status else out[:n]

    def debug_numa_merge(self, cases: np.ndarray) -> np.ndarray:
        """The device topology-manager policy merge on int64[n, DBG_MERGE_WORDS] cases (kg_debug_numa_merge);
        returns int64[n, 8]: admit, nil, mask, preferred, score."""
        cases = np.ascontiguousarray(cases, dtype=np.int64).reshape(-1, abi.DBG_MERGE_WORDS)
        out = np.zeros((len(cases), 8), dtype=np.int64)
        check(self.lib, self.lib.kg_debug_numa_merge(self.h, ptr(cases), len(cases), ptr(out)))
        return out

    def debug_least_requested(self, requested, capacity):
        requested = np.ascontiguousarray(requested, dtype=np.int64)
        capacity = np.ascontiguousarray(capacity, dtype=np.int64)
        out = np.zeros(len(requested), dtype=np.int64)
        check(self.lib, self.lib.kg_debug_least_requested(self.h, ptr(requested), ptr(capacity), ptr(out),
                                                          len(requested)))
        return out

    def debug_fast_lrs(self, requested, capacity):
        """(cpu-routine, memory-routine) leastRequestedScore of the wide pass; -1 outside a routine's domain."""
        requested = np.ascontiguousarray(requested, dtype=np.int64)
        capacity = np.ascontiguousarray(capacity, dtype=np.int64)
        oc = np.zeros(len(requested), dtype=np.int64)
        om = np.zeros(len(requested), dtype=np.int64)
        check(self.lib, self.lib.kg_debug_fast_lrs(self.h, ptr(requested), ptr(capacity), ptr(oc), ptr(om),
                                                   len(requested)))
        return oc, om

    # -- NodeResourcesFit RequestedToCapacityRatio -----------------------------------------------------------------
    def set_fit_shape(self, points):
        """Score NodeResourcesFit by RequestedToCapacityRatio with this shape: (utilization, score) pairs or an array of
        abi.SHAPE_POINT_DTYPE.  None or an empty shape returns to the configured strategy.  The engine validates."""
        if points is None:
            points = []
        if isinstance(points, np.ndarray) and points.dtype == abi.SHAPE_POINT_DTYPE:
            arr = np.ascontiguousarray(points)
        else:
            arr = np.array([(int(u), int(s)) for u, s in points], dtype=abi.SHAPE_POINT_DTYPE)
        check(self.lib, self.lib.kg_fit_shape_set(self.h, ptr(arr) if len(arr) else None, len(arr)))

    def fit_shape(self):
        """(the table raw(0..100) the engine scores with, whether RequestedToCapacityRatio is active)."""
        lut = np.zeros(101, dtype=np.int64)
        active = ctypes.c_int64(0)
        check(self.lib, self.lib.kg_fit_shape_get(self.h, ptr(lut), ctypes.byref(active)))
        return lut, bool(active.value)

    def debug_fit_shape(self, requested, capacity):
        """(reference-shaped, cpu-routine, memory-routine) per-resource shape score; a fast routine gives -1 outside its
        domain."""
        requested = np.ascontiguousarray(requested, dtype=np.int64)
        capacity = np.ascontiguousarray(capacity, dtype=np.int64)
        ref = np.zeros(len(requested), dtype=np.int64)
        oc = np.zeros(len(requested), dtype=np.int64)
        om = np.zeros(len(requested), dtype=np.int64)
        check(self.lib, self.lib.kg_debug_fit_shape(self.h, ptr(requested), ptr(capacity), ptr(ref), ptr(oc), ptr(om),
                                                    len(requested)))
        return ref, oc, om

    def debug_balanced(self, alloc, requested, pod, resources=3):
        """NodeResourcesBalancedAllocation's score of n (Allocatable, Requested, pod request) triples, each argument an
        (n, 2) array of (cpu, memory): (reference-shaped, round engine's hoisted form); the second gives -1 outside its
        exact domain."""
        cols = [np.ascontiguousarray(np.asarray(a, dtype=np.int64).reshape(-1, 2).T) for a in (alloc, requested, pod)]
        n = cols[0].shape[1]
        if any(c.shape[1] != n for c in cols):
            raise ValueError("alloc, requested and pod must hold the same number of (cpu, memory) pairs")
        ref = np.zeros(n, dtype=np.int64)
        hot = np.zeros(n, dtype=np.int64)
        check(self.lib, self.lib.kg_debug_balanced(self.h, ptr(cols[0]), ptr(cols[1]), ptr(cols[2]), int(resources),
                                                   ptr(ref), ptr(hot), n))
        return ref, hot

    def debug_fast_mrs(self, requested, capacity):
        """(reference-shaped, cpu-routine, memory-routine) mostRequestedScore; a fast routine gives -1 outside its domain."""
        requested = np.ascontiguousarray(requested, dtype=np.int64)
        capacity = np.ascontiguousarray(capacity, dtype=np.int64)
        ref = np.zeros(len(requested), dtype=np.int64)
        oc = np.zeros(len(requested), dtype=np.int64)
        om = np.zeros(len(requested), dtype=np.int64)
        check(self.lib, self.lib.kg_debug_fast_mrs(self.h, ptr(requested), ptr(capacity), ptr(ref), ptr(oc), ptr(om),
                                                   len(requested)))
        return ref, oc, om
