// kg_debug_topn (ABI 18): the top-N per-plugin score table of one pod, ranked on the device — what koord-scheduler's
// --debug-scores prints (frameworkext/debug.go:61-108) without copying an n-row vector per plugin to the host.
//
// Four plain launches on the engine stream, in stream order (no spin on another kernel, no cooperative
// launch), over scratch of their own (the engine's topn_buf): nothing a schedule call reads later is written.
//   topn_eval    one thread per node: rsv_eval_node — the per-node body of the exact pass, which also serves single-pod
//                schedule calls of every profile (wide, NodeNUMAResource only, DeviceShare only, exact) — packed with
//                rsv_pack into val[i]; per-block partials in the scheduling pass's part[] layout (part[b] preferred
//                node, part[nb + b] max raw Reservation Score, part[3 nb + b] max raw DeviceShare Score, part[4 nb + b]
//                / part[5 nb + b] max raw TaintToleration / NodeAffinity Score), and part[2 nb + b] = the block's
//                feasible count (the scheduling pass keeps its block key there; this pass ranks N keys, not one).
//   topn_select  select_key — rsv_select's weighted total (rsv_total against the maxima) packed with make_key — per
//                node; each block keeps its best `topn` keys: block max, then the max below it, `topn` times (keys are
//                unique, so "below the last one" knocks the earlier winners out without a store).
//   topn_final   one block reduces the nb · topn candidates to the final `topn` the same way and sums the feasible count.
//   topn_gather  one thread per winner evaluates its node again with RsvDbg and writes the kg_topn_row: the weighted
//                parts of `base` as rsv_eval_node names them, and each normalised plugin's share as rsv_total computes it
//                with every other plugin switched off (so the columns are the scheduler's formula, not a copy of it).
// Included by engine.hip after rsv_dev.h, as xr_dev.h is.
#pragma once

constexpr int kTopnFinalThreads = 1024;  // 16 waves over ≤ nb · KG_TOPN_MAX candidates

// header of the call's output buffer, copied back with the rows in one transfer
struct TopnHdr {
  int64_t n_rows, feasible;
};

__global__ __launch_bounds__(kRsvThreads) void topn_eval(DevTable T, const RsvNode* __restrict__ RN,
                                                         const int32_t* __restrict__ rsv_n,
                                                         const LonePod* __restrict__ lp, uint32_t on, int64_t n,
                                                         EvalParams P, RsvParams RP, RsvExt X,
                                                         uint64_t* __restrict__ val, uint64_t* __restrict__ part) {
  __shared__ uint64_t s_red[kRsvThreads / kWave];
  const int nb = gridDim.x;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t v = 0, pk = 0, rawv = 0, dsv = 0, tv = 0, av = 0;
  if (i < n) {
    const LoneArgs a = lone_args(*lp, on, X);
    const RsvOut o = rsv_eval_node(T, RN, rsv_n, i, lp->pod, lp->rpod, P, RP, a.X, a.dpod, a.npod, nullptr, a.aux, a.df);
    if (o.feas) {
      v = rsv_pack(o);
      pk = rsv_pref_key(o, (uint32_t)i);
      rawv = (uint64_t)(uint32_t)o.raw;
      dsv = (uint64_t)(uint32_t)o.dsraw;
      tv = (uint64_t)(uint32_t)o.tcnt;
      av = (uint64_t)(uint32_t)o.asum;
    }
    val[i] = v;
    if (X.val2) X.val2[i] = (uint32_t)(tv << 24 | av);
  }
  const uint64_t fc = rsv_block_sum(v ? 1u : 0u, s_red);
  __syncthreads();
  pk = rsv_block_max(pk, s_red);
  __syncthreads();
  rawv = rsv_block_max(rawv, s_red);
  __syncthreads();
  dsv = rsv_block_max(dsv, s_red);
  __syncthreads();
  tv = rsv_block_max(tv, s_red);
  __syncthreads();
  av = rsv_block_max(av, s_red);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = pk;
    part[nb + blockIdx.x] = rawv;
    part[2 * nb + blockIdx.x] = fc;
    part[3 * nb + blockIdx.x] = dsv;
    part[4 * nb + blockIdx.x] = tv;
    part[5 * nb + blockIdx.x] = av;
  }
}

// cand[b · topn + r] = block b's r-th best key (0 past its feasible nodes)
__global__ __launch_bounds__(kRsvThreads) void topn_select(const uint64_t* __restrict__ val, int64_t n, int topn,
                                                           RsvParams RP, RsvExt X, const uint64_t* __restrict__ part,
                                                           uint64_t* __restrict__ cand) {
  __shared__ uint64_t s_red[kRsvThreads / kWave];
  __shared__ uint64_t s_best;
  const int nb = gridDim.x;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t key = select_key(val, i, n, nb, RP, X, part);
  uint64_t* out = cand + (size_t)blockIdx.x * topn;
  uint64_t prev = ~0ull;
  for (int r = 0; r < topn; ++r) {  // uniform: every thread reads the same s_best
    const uint64_t m = rsv_block_max(key < prev ? key : 0, s_red);
    if (threadIdx.x == 0) {
      s_best = m;
      out[r] = m;
    }
    __syncthreads();
    prev = s_best;
    if (prev == 0) {
      if (threadIdx.x == 0)
        for (int q = r + 1; q < topn; ++q) out[q] = 0;
      break;
    }
  }
}

// win[r] = the r-th best key over all candidates; hdr = {rows, feasible nodes}
__global__ __launch_bounds__(kTopnFinalThreads) void topn_final(const uint64_t* __restrict__ cand, int64_t n_cand,
                                                                int nb, int topn, const uint64_t* __restrict__ part,
                                                                uint64_t* __restrict__ win, TopnHdr* __restrict__ hdr) {
  __shared__ uint64_t s_red[kTopnFinalThreads / kWave];
  __shared__ uint64_t s_best;
  const uint64_t feasible = rsv_partials_sum(part + 2 * nb, nb);  // every wave, every lane
  uint64_t prev = ~0ull;
  int rows = 0;
  for (int r = 0; r < topn; ++r) {
    uint64_t m = 0;
    for (int64_t k = threadIdx.x; k < n_cand; k += kTopnFinalThreads) {
      const uint64_t c = cand[k];
      if (c < prev && c > m) m = c;
    }
    m = wave_max_u64_dpp(m);
    if ((threadIdx.x & (kWave - 1)) == 0) s_red[threadIdx.x / kWave] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int k = 1; k < kTopnFinalThreads / kWave; ++k) m = s_red[k] > m ? s_red[k] : m;
      s_best = m;
      win[r] = m;
    }
    __syncthreads();
    prev = s_best;
    if (prev == 0) break;
    ++rows;
  }
  if (threadIdx.x == 0) {
    hdr->n_rows = rows;
    hdr->feasible = (int64_t)feasible;
  }
}

// `en` = bit KG_PL_*: the plugin is enabled at Score in the profile (the others' columns are -1)
__global__ __launch_bounds__(kWave) void topn_gather(DevTable T, const RsvNode* __restrict__ RN,
                                                     const int32_t* __restrict__ rsv_n,
                                                     const LonePod* __restrict__ lp, uint32_t on, int nb,
                                                     EvalParams P, RsvParams RP, RsvExt X,
                                                     const uint64_t* __restrict__ part,
                                                     const uint64_t* __restrict__ win,
                                                     const TopnHdr* __restrict__ hdr, uint32_t en,
                                                     kg_topn_row* __restrict__ rows) {
  // the maxima, as select_key reads them (every lane of the one wave)
  const uint64_t pk = rsv_partials_max(part, nb);
  const uint64_t mraw = rsv_partials_max(part + nb, nb);
  const int64_t mds = X.ds ? (int64_t)rsv_partials_max(part + 3 * nb, nb) : 0;
  const int64_t mt = X.val2 ? (int64_t)rsv_partials_max(part + 4 * nb, nb) : 0;
  const int64_t ma = X.val2 ? (int64_t)rsv_partials_max(part + 5 * nb, nb) : 0;
  const int64_t pref = pk ? (int64_t)(uint32_t)(~pk) : -1;
  const int64_t mx = pk ? (mraw > 1000 ? (int64_t)mraw : 1000) : (int64_t)mraw;
  const int r = threadIdx.x;
  if (r >= hdr->n_rows) return;
  const uint64_t key = win[r];
  const int64_t i = (int64_t)key_node(key);
  RsvDbg d;
  const LoneArgs a = lone_args(*lp, on, X);
  const RsvOut o = rsv_eval_node(T, RN, rsv_n, i, lp->pod, lp->rpod, P, RP, a.X, a.dpod, a.npod, &d, a.aux, a.df);
  kg_topn_row row;
  row.node_idx = (int32_t)i;
  row.nominated = o.feas ? o.nom : -1;
  row.total = (int64_t)(key >> 32);
#pragma unroll
  for (int c = 0; c < KG_PL_COLUMNS; ++c) row.plugin[c] = -1;
  // the normalised plugins: rsv_total of the node's packed value without `base`, one plugin switched on at a time
  const uint64_t vb = rsv_pack(o) & 0xFFFFFFFFull;
  const uint32_t v2 = (uint32_t)o.tcnt << 24 | (uint32_t)o.asum;
  RsvParams R0 = RP;
  R0.score = 0;
  RsvExt X0 = X;
  X0.DP.score = 0, X0.DF.taint_score = 0, X0.DF.aff_score = 0;
  if (en >> KG_PL_FIT & 1u) row.plugin[KG_PL_FIT] = d.w_fit;
  if (en >> KG_PL_LOADAWARE & 1u) row.plugin[KG_PL_LOADAWARE] = d.w_la;
  if (en >> KG_PL_NUMA & 1u) row.plugin[KG_PL_NUMA] = d.w_numa;
  if (en >> KG_PL_BALANCED & 1u) row.plugin[KG_PL_BALANCED] = d.w_bal;
  if (en >> KG_PL_IMAGE_LOCALITY & 1u) row.plugin[KG_PL_IMAGE_LOCALITY] = d.w_img;
  if (en >> KG_PL_RESERVATION & 1u) row.plugin[KG_PL_RESERVATION] = rsv_total(vb, v2, i == pref, mx, 0, 0, 0, RP, X0);
  if (en >> KG_PL_DEVICESHARE & 1u) {
    RsvExt X1 = X0;
    X1.DP.score = X.DP.score;
    row.plugin[KG_PL_DEVICESHARE] = rsv_total(vb, v2, false, 0, mds, 0, 0, R0, X1);
  }
  if (en >> KG_PL_TAINT & 1u) {
    RsvExt X1 = X0;
    X1.DF.taint_score = X.DF.taint_score;
    row.plugin[KG_PL_TAINT] = rsv_total(vb, v2, false, 0, 0, mt, 0, R0, X1);
  }
  if (en >> KG_PL_NODE_AFFINITY & 1u) {
    RsvExt X1 = X0;
    X1.DF.aff_score = X.DF.aff_score;
    row.plugin[KG_PL_NODE_AFFINITY] = rsv_total(vb, v2, false, 0, 0, 0, ma, R0, X1);
  }
  rows[r] = row;
}

