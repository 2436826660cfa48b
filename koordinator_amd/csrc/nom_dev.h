// Nominated pods on the device (added within ABI 18): the resident nominated-pod table and the rule
// of upstream's RunFilterPluginsWithNominatedPods / addNominatedPods (k8s v1.24.15 framework/runtime/framework.go,
// restated as published, parity-unpinned): before a pod of priority q is filtered on node n, every nominated pod on n
// with priority >= q and another uid is added to the node (NodeInfo.AddPod); Filters must pass on that augmented node
// and, when anything was added, on the plain node too.
//
// Only two accelerated Filters read what AddPod changes — NodeResourcesFit (Requested of every resource and the pod
// count) and NodeNUMAResource's filterAmplifiedCPUs (Requested.MilliCPU) — and both can only turn from pass to reject
// when Requested grows.  So the feasible set is the plain Filter AND (those two on the augmented row): nom_fits.
// Scores are computed from the plain row.
//
// The table is a structure of arrays sorted by (node, priority descending), so the entries a pod sees on a node are a
// prefix of the node's run; first[node] = 1 + the run's first entry, 0 = the node has none.  An entry dies (live = 0)
// when the engine places the pod with its uid; the flag is written by rsv_apply / the Reserve of a call's last pod,
// when no other wave of the launch reads it (nom_placed).
// Included by rsv_dev.h (RsvExt carries the view) and through it by engine.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/koordgpu.h"
#include "kernels.h"
#include "numa_dev.h"
#include "round_ctl.h"

namespace kg {

constexpr int kNomRes = 2 + kAux;  // cpu, memory, then the kAux resources: the requests kg_pods_add reads

struct NomView {
  const int32_t* __restrict__ node;  // [n]
  const int32_t* __restrict__ prio;  // [n] PodPriority
  const int64_t* __restrict__ uid;   // [n]
  int32_t* live;                     // [n] 1 = in the nominator, 0 = removed by placement
  const int64_t* __restrict__ req;   // [kNomRes][n]
  int32_t n;
  int32_t pad;
};

// what addNominatedPods adds to one node for one pod
struct NomSum {
  int64_t cpu, mem;
  int64_t aux[kAux];
  int32_t k;  // entries added (the pod count grows by k; an all-zero entry still counts)
};

// One thread walks one node's run: first1 = first[node] (non-zero).  The run is sorted by priority descending, so the
// walk stops at the first entry below the pod's priority.
__device__ __forceinline__ NomSum nom_sum(const NomView& V, int32_t first1, int64_t node, int32_t prio, int64_t uid) {
  NomSum s{};
  for (int32_t e = first1 - 1; e < V.n && V.node[e] == node && V.prio[e] >= prio; ++e) {
    if (!V.live[e] || V.uid[e] == uid) continue;
    s.cpu += V.req[e];
    s.mem += V.req[(size_t)V.n + e];
#pragma unroll
    for (int q = 0; q < kAux; ++q) s.aux[q] += V.req[(size_t)(2 + q) * V.n + e];
    s.k += 1;
  }
  return s;
}

// NodeResourcesFit's fitsRequest (ephemeral-storage and the scalar resources included) and filterAmplifiedCPUs on node
// i's row with `s` added: 0 = both pass, else the KG_REJECT_FIT_* / KG_REJECT_NUMA bits.  aux_req: the pod's kAux
// requests (nullable = none); nv / np: the node's NUMA view and the pod's NUMA record (nullable = the plugin is not at
// Filter in the profile).  eval_node, aux_fits and numa_amp_cpu_fits are the scheduling passes' own.
__device__ __forceinline__ uint32_t nom_fits(const DevTable& T, int64_t i, const Row& r, const DevPod& p,
                                             const int64_t* aux_req, const EvalParams& P, const NomSum& s,
                                             const NumaView* nv, const NumaPod* np) {
  constexpr uint32_t kFit = KG_REJECT_FIT_PODS | KG_REJECT_FIT_CPU | KG_REJECT_FIT_MEMORY | KG_REJECT_FIT_OTHER;
  Row a = r;
  a.req_cpu += s.cpu;
  a.req_mem += s.mem;
  a.num_pods += s.k;
  if (T.aux) {  // ephemeral-storage Requested > Allocatable rejects every pod with a non-zero request
    const bool over = T.aux[(size_t)kAux * T.cap + i] + s.aux[0] > T.aux[i];
    a.flags = (a.flags & ~F_EPH_OVER) | (over ? F_EPH_OVER : 0u);
  }
  EvalParams Q = P;  // the Filter verdicts only
  Q.fit_score = Q.la_score = Q.la_filter = 0;
  uint32_t rej = 0;
  int64_t t = 0;
  (void)eval_node(a, p, Q, t, &rej);
  rej &= kFit;
  if (aux_req && P.fit_filter && T.aux && !aux_fits(T, i, aux_req, s.aux)) rej |= KG_REJECT_FIT_OTHER;
  if (nv && np && !numa_amp_cpu_fits(*nv, *np, a.req_cpu, a.alloc_cpu)) rej |= KG_REJECT_NUMA;
  return rej;
}

// The pod a schedule call's last Reserve placed was nominated: its entry leaves the table.  ws[WS_NOM_KILL] = 1 + the
// entry the host found for the call's last pod (0 = that pod is not in the table).  Called by the one thread that ran
// the Reserve, from rsv_apply (a one-wave launch of its own) or from the pass after the call's last pod, which
// evaluates no node: no wave of the launch reads the flag.  An ordinary vector store.
__device__ __forceinline__ void nom_placed(const NomView& V, const unsigned long long* __restrict__ ws) {
  const unsigned long long k = ws[WS_NOM_KILL];
  if (k != 0 && k <= (unsigned long long)V.n) V.live[k - 1] = 0;
}

// kg_pods_filter_nominated: per node, the augmented pass's reject bits and how many entries were added
constexpr int kNomThreads = 256;
__global__ __launch_bounds__(kNomThreads) void nom_filter(DevTable T, int64_t n, const DevPod* __restrict__ pod,
                                                          const int64_t* __restrict__ pod_aux,
                                                          const NumaPod* __restrict__ npod,
                                                          const NumaStatic* __restrict__ ns,
                                                          const NumaMut* __restrict__ nm, NumaParams NP, EvalParams P,
                                                          const int32_t* __restrict__ first, NomView V, int32_t prio,
                                                          int64_t uid, int32_t* __restrict__ out_reject,
                                                          int32_t* __restrict__ out_added) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const DevPod p = *pod;
  const Row r = load_row(T, i);
  const int32_t f1 = first ? first[i] : 0;
  const NomSum s = f1 ? nom_sum(V, f1, i, prio, uid) : NomSum{};
  int64_t rq[kAux];
#pragma unroll
  for (int q = 0; q < kAux; ++q) rq[q] = pod_aux[q];
  uint32_t rej;
  if (ns && NP.filter) {
    const NumaView v = make_view(ns + i, nm + i, NP);
    const NumaPod np = *npod;
    rej = nom_fits(T, i, r, p, (p.flags & P_AUX) ? rq : nullptr, P, s, &v, &np);
  } else {
    rej = nom_fits(T, i, r, p, (p.flags & P_AUX) ? rq : nullptr, P, s, nullptr, nullptr);
  }
  out_reject[i] = (r.flags & F_VALID) ? (int32_t)rej : (int32_t)KG_REJECT_INVALID_NODE;
  out_added[i] = s.k;
}

}  // namespace kg
