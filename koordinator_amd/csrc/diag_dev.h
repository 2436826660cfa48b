// kg_pods_diagnose (added within ABI 18): framework.FitError of many pods per call, reduced on the device — per pod
// NumAllNodes, the feasible count, the NodeToStatusMap reasons histogram and the nodes per first-failing plugin
// (Diagnosis.UnschedulablePlugins), a few hundred bytes, instead of an n-row vector per plugin copied to the host.
//
// Two plain launches per chunk of pods on the engine stream, in stream order (no spin on another kernel, no
// cooperative launch, no atomics on the result), over scratch of their own (the engine's diag_buf): nothing a schedule
// call reads later is written.
//   diag_eval    one thread per node, blocks of kRsvThreads; grid (node blocks, pod groups).  A block loops over the
//                pods of its group (pod j = blockIdx.y, += gridDim.y: with one group this is the plain pod loop, with as
//                many groups as pods the 2-D grid; the host sizes the groups to fill the device).  The pod index is
//                block-uniform, so the pod records (one LonePod per pod) come through scalar loads.  Per pod the
//                thread runs rsv_eval_node — the scheduler's per-node body — with a status pointer, which makes it evaluate every Filter and report
//                the framework's first failure (rsv_status).  Per counter one ballot + population count per wave; the
//                waves combine through LDS (double-buffered by the loop's parity: one barrier per pod) and the block
//                stores one partial row part[pod][block][kDiagRow].  With a status buffer each thread stores its word.
//   diag_final   one block per pod sums the pod's `nb` partial rows into its kg_fit_diag.  Integer sums over stored
//                partials are order-independent: the result is bit-reproducible.
// Included by engine.hip after topn_dev.h.
#pragma once

constexpr int kDiagReasons = 10;                  // the KG_REJECT_* bits a Filter status can carry
constexpr int kDiagCnt = 3 + kDiagReasons;        // valid slots, feasible, NodeResourcesFit nodes, one per reason bit
constexpr int kDiagRow = 16;                      // words per partial row
constexpr int kDiagFinalThreads = 256;            // kDiagRow counters × 16 strided block groups
constexpr int kDiagChunk = 64;                    // pods per diag_eval launch (bounds the partials and the status words)
constexpr int kDiagFillBlocks = 2048;             // blocks a launch aims for: 8 per CU of a 256-CU device
constexpr uint32_t kDiagFitBits = KG_REJECT_FIT_PODS | KG_REJECT_FIT_CPU | KG_REJECT_FIT_MEMORY | KG_REJECT_FIT_OTHER;
// counter 3 + k counts the nodes whose status carries bit diag_bit(k)
__host__ __device__ constexpr int diag_bit(int k) {
  return k == 0 ? 0 : k == 1 ? 1 : k == 2 ? 2 : k == 3 ? 3 : k == 4 ? 5 : k == 5 ? 6 : k == 6 ? 7 : k == 7 ? 8 : k == 8 ? 12 : 13;
}
static_assert((1u << diag_bit(3)) == KG_REJECT_LOADAWARE && (1u << diag_bit(4)) == KG_REJECT_NUMA &&
              (1u << diag_bit(5)) == KG_REJECT_DEVICE && (1u << diag_bit(6)) == KG_REJECT_FIT_OTHER &&
              (1u << diag_bit(7)) == KG_REJECT_RESERVATION && (1u << diag_bit(8)) == KG_REJECT_TAINT &&
              (1u << diag_bit(9)) == KG_REJECT_NODE_AFFINITY, "diag reason bits");
static_assert(kDiagCnt <= kDiagRow && KG_DIAG_REASONS == 32, "diag row");

__global__ __launch_bounds__(kRsvThreads) void diag_eval(DevTable T, const RsvNode* __restrict__ RN,
                                                         const int32_t* __restrict__ rsv_n,
                                                         const LonePod* __restrict__ pods, int n_pods, int64_t n,
                                                         EvalParams P, RsvParams RP, RsvExt X, uint32_t on,
                                                         uint32_t* __restrict__ part, int32_t* __restrict__ status) {
  __shared__ uint32_t s_cnt[2][kRsvThreads / kWave][kDiagRow];
  const int nb = gridDim.x;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  int par = 0;
  for (int j = blockIdx.y; j < n_pods; j += gridDim.y, par ^= 1) {  // uniform over the block
    const LonePod& q = pods[j];
    uint32_t w = KG_REJECT_INVALID_NODE;  // rows past the table count nowhere, like invalid slots
    if (i < n) {
      const LoneArgs a = lone_args(q, on, X);
      w = 0;
      rsv_eval_node(T, RN, rsv_n, i, q.pod, q.rpod, P, RP, a.X, a.dpod, a.npod, nullptr, a.aux, a.df, &w);
      if (status) status[(size_t)j * (size_t)n + (size_t)i] = (int32_t)w;
    }
    const bool valid = w != KG_REJECT_INVALID_NODE;
    uint32_t c[kDiagCnt];
    c[0] = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(valid));
    c[1] = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(w == 0));
    c[2] = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(valid && (w & kDiagFitBits) != 0));
#pragma unroll
    for (int k = 0; k < kDiagReasons; ++k)
      c[3 + k] = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(valid && ((w >> diag_bit(k)) & 1u) != 0));
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < kDiagCnt; ++k) s_cnt[par][wave][k] = c[k];
    }
    // one barrier per pod: the next iteration writes the other half, and a thread reaches the iteration after that
    // only through the next barrier, which every reader of this half has passed its reads to reach
    __syncthreads();
    if (threadIdx.x < kDiagRow) {
      uint32_t v = 0;
      if (threadIdx.x < kDiagCnt) {
#pragma unroll
        for (int k = 0; k < kRsvThreads / kWave; ++k) v += s_cnt[par][k][threadIdx.x];
      }
      part[((size_t)j * nb + blockIdx.x) * kDiagRow + threadIdx.x] = v;
    }
  }
}

__global__ __launch_bounds__(kDiagFinalThreads) void diag_final(const uint32_t* __restrict__ part, int nb,
                                                                kg_fit_diag* __restrict__ out) {
  constexpr int kGroups = kDiagFinalThreads / kDiagRow;
  __shared__ int64_t s_sum[kGroups][kDiagRow];
  const int j = blockIdx.x, k = threadIdx.x & (kDiagRow - 1), g = threadIdx.x / kDiagRow;
  int64_t v = 0;
  for (int b = g; b < nb; b += kGroups) v += part[((size_t)j * nb + b) * kDiagRow + k];
  s_sum[g][k] = v;
  __syncthreads();
  if (threadIdx.x != 0) return;
  int64_t c[kDiagCnt];
#pragma unroll
  for (int q = 0; q < kDiagCnt; ++q) {
    int64_t t = 0;
    for (int h = 0; h < kGroups; ++h) t += s_sum[h][q];
    c[q] = t;
  }
  kg_fit_diag d;
  d.num_all_nodes = c[0];
  d.feasible = c[1];
#pragma unroll
  for (int q = 0; q < KG_PL_COLUMNS; ++q) d.plugin_nodes[q] = 0;
#pragma unroll
  for (int q = 0; q < KG_DIAG_REASONS; ++q) d.reason_nodes[q] = 0;
#pragma unroll
  for (int q = 0; q < kDiagReasons; ++q) d.reason_nodes[diag_bit(q)] = c[3 + q];
  d.plugin_nodes[KG_PL_FIT] = c[2];
  d.plugin_nodes[KG_PL_LOADAWARE] = c[3 + 3];
  d.plugin_nodes[KG_PL_NUMA] = c[3 + 4];
  d.plugin_nodes[KG_PL_DEVICESHARE] = c[3 + 5];
  d.plugin_nodes[KG_PL_RESERVATION] = c[3 + 7];
  d.plugin_nodes[KG_PL_TAINT] = c[3 + 8];
  d.plugin_nodes[KG_PL_NODE_AFFINITY] = c[3 + 9];
  out[j] = d;
}
