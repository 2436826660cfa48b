// What the round engine's serial NUMA and DeviceShare resolvers and Unreserve do per pod, written once: the pick of
// the pod's first unmodified candidate, the search for the lane that owns the winner, the load of a node into a NUMA
// slot, and the nine NodeInfo.AddPod / LoadAware assign-cache terms a placement adds onto the node's Row.
// DESIGN.md §3.23 says who calls each and which resolvers keep their own text.  Included by engine.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "numa_dev.h"
#include "round_ctl.h"

namespace kg {

// ---- what a placement commits --------------------------------------------------------------------------------------
// assume(pod) on a node's Row: NodeInfo.AddPod + LoadAware Reserve → podAssignCache.assign (load_aware.go:260-263);
// sign = -1 is the framework's Unreserve (NodeInfo.RemovePod + unAssign, pod_assign_cache.go:119-131)
__device__ __forceinline__ void row_assume(Row& r, const DevPod& p, int64_t sign = 1) {
  const int64_t prod = (p.flags & P_PROD) ? sign : 0;
  r.req_cpu += sign * p.req_cpu;
  r.req_mem += sign * p.req_mem;
  r.nz_cpu += sign * p.nz_cpu;
  r.nz_mem += sign * p.nz_mem;
  r.la_used_cpu += sign * p.est_cpu;
  r.la_used_mem += sign * p.est_mem;
  r.la_pused_cpu += prod * p.est_cpu;
  r.la_pused_mem += prod * p.est_mem;
  r.num_pods += (int32_t)sign;
}

// ---- the pod's candidates and the modified rows --------------------------------------------------------------------
// the modified-row bitmap (LDS, one bit per node)
__device__ __forceinline__ bool bm_test(const uint32_t* bitmap, uint32_t node) {
  return (bitmap[node >> 5] >> (node & 31)) & 1u;
}
__device__ __forceinline__ void bm_set(uint32_t* bitmap, uint32_t node) { bitmap[node >> 5] |= 1u << (node & 31); }

// The first listed candidate whose node no pod has modified: lane l holds the pod's l-th key (0 = none).  mask = the
// lanes with an unmodified candidate, pos = the first of them (kWave when there is none: one candidate per lane, so
// kC), key = its key (0).  Wave-uniform.
struct FirstUnmod {
  uint64_t mask;
  int pos;
  uint64_t key;
};
__device__ __forceinline__ FirstUnmod first_unmodified(uint64_t key, const uint32_t* bitmap) {
  const bool unmod = key != 0 && !bm_test(bitmap, key_node(key));
  const uint64_t um = __ballot(unmod);
  const int pos = um ? (int)__builtin_ctzll(um) : kWave;
  return FirstUnmod{um, pos, um ? readlane_u64(key, pos) : 0};
}

// The lane that owns winner w: lane l < nM holds modified node slot_node, so w is either one of those or the best
// unmodified candidate, which takes the spare slot nM and is marked in the bitmap here (fresh).  The caller then grows
// its own nM.  Wave-uniform.
struct SlotOwner {
  int lane;
  bool fresh;
};
__device__ __forceinline__ SlotOwner slot_owner(int lane, uint32_t slot_node, int nM, uint32_t w, uint32_t* bitmap) {
  const uint64_t hit = __ballot(lane < nM && slot_node == w);
  if (!hit && lane == 0) bm_set(bitmap, w);
  return SlotOwner{hit ? (int)__builtin_ctzll(hit) : nM, !hit};
}

// ---- staging -------------------------------------------------------------------------------------------------------
// A node into a NUMA resolver slot: its Row, its NumaStatic / NumaMut (tables ns_tab / nm_tab) into the slot's LDS
// records ns / nm, and the view built from those
__device__ __forceinline__ void numa_slot_load(const DevTable& T, const NumaStatic* ns_tab, const NumaMut* nm_tab,
                                               uint32_t node, const NumaParams& NP, Row& row, NumaStatic* ns,
                                               NumaMut* nm, NumaView& view) {
  row = load_row(T, node);
  *ns = ns_tab[node];
  *nm = nm_tab[node];
  view = make_view(ns, nm, NP);
}

}  // namespace kg
