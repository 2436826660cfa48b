// The resolvers' dynamic LDS: one layout per kernel, built by one __host__ __device__ function of the run-time
// quantities the carve depends on.  The kernel takes its section pointers from the layout, the launch its size
// (bytes()), prepare_rounds its check against kMaxLds — the same function with the same arguments, so the three cannot
// drift.  An LDS access past the allocation does not fault (reads return zero, writes are dropped): a wrong size would
// lose the tail of the last section, the modified-row bitmap, and place pods wrongly instead of crashing.
// DESIGN.md §3.3 / §3.4.  Included by engine.hip; xr_dev.h is compiled inside engine.hip and sees it from there.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/koordgpu.h"
#include "ds_dev.h"
#include "kernels.h"
#include "numa_dev.h"
#include "round_ctl.h"
#include "rsv_dev.h"

namespace kg {

constexpr size_t kMaxLds = 160 * 1024;  // LDS of one workgroup (gfx950): what a resolver launch may ask for
constexpr int64_t kMaxNodes = 1 << 19;  // a resolver's bitmap holds one bit per node (static_asserts below)
constexpr int kMaxDsB = 32;             // pods per DeviceShare round (kg_config.batch_pods of a DeviceShare profile)
constexpr int kXrPods = 32;             // pods per exact round (< kWave: one modified row per resolver lane)

// a pod's merged record (merge_round's output, a resolver's input), in uint64 words
constexpr int kC = 64;            // merged candidates per pod (> any modified-set size: kC > kMaxB - 1)
constexpr int kStaged = 3;        // hoisted rows of each pod's best candidates shipped with its record
constexpr int kRecRows = 72;      // [0,kC) keys, [kC] ub, [72, 72 + kStaged·kEvalRowWords) rows
constexpr int kCandStride = 128;  // per-pod record: 1 KiB (a 16-B multiple, for LDS-DMA)
constexpr int kR = 8;             // candidates kept per (pod, tile)
static_assert(kRecRows + kStaged * kEvalRowWords <= kCandStride, "record layout");
static_assert(kCandStride % 2 == 0 && kPodWords % 2 == 0, "records and pods in whole 16-byte LDS-DMA transfers");

// the staged records in 8-byte words (the prologues copy them word by word)
constexpr int kParWords = (int)((sizeof(EvalParams) + 7) / 8);
constexpr int kRowWords = (int)(sizeof(Row) / 8);
constexpr int kNumaStaticWords = (int)(sizeof(NumaStatic) / 8), kNumaMutWords = (int)(sizeof(NumaMut) / 8);
constexpr int kNumaPodWords = (int)(sizeof(NumaPod) / 8), kViewWords = (int)(sizeof(NumaView) / 8);
constexpr int kDsPodWords = (int)(sizeof(DsPod) / 8);
constexpr int kRsvPodWords = (int)(sizeof(RsvPod) / 8), kDefPodWords = (int)((sizeof(DefPod) + 7) / 8);
static_assert(sizeof(Row) % 8 == 0 && sizeof(NumaView) % 8 == 0 && sizeof(NumaStatic) % 8 == 0 &&
                  sizeof(NumaMut) % 8 == 0 && sizeof(NumaPod) % 8 == 0 && sizeof(DsNode) % 8 == 0 &&
                  sizeof(DsPod) % 8 == 0 && sizeof(RsvPod) % 8 == 0 && sizeof(QuotaRow) % 8 == 0,
              "staged records in 8-byte words");

// Carves consecutive sections out of a kernel's dynamic LDS, in the idiom of the host's Carver: take<T>(count) is the
// byte offset of the next section, aligned to kAlign (alignof(T) unless the call states more: the target of a 16-byte
// global_load_lds transfer or of uint4 stores says 16); bytes() is the end of the last section.
struct LdsCarver {
  uint32_t n = 0;
  template <typename T, uint32_t kAlign = alignof(T)>
  __host__ __device__ constexpr uint32_t take(uint32_t count) {
    static_assert(kAlign >= alignof(T) && (kAlign & (kAlign - 1)) == 0 && kAlign <= 16,
                  "a power of two, at most the 16 bytes the kernels align smem to");
    n = (n + kAlign - 1) & ~(kAlign - 1);
    const uint32_t at = n;
    n += count * (uint32_t)sizeof(T);
    return at;
  }
  __host__ __device__ constexpr uint32_t bytes() const { return n; }
};
template <typename T>
__device__ __forceinline__ T* lds_at(uint64_t* smem, uint32_t offset) {
  return reinterpret_cast<T*>(reinterpret_cast<char*>(smem) + offset);
}

// A prologue's plain copy of the round's nb records of `words` 8-byte words, src[first, first + nb), to their section
__device__ __forceinline__ void lds_stage(uint64_t* dst, const void* src, int64_t first, int nb, int words, int tid,
                                          int threads) {
  const uint64_t* g = reinterpret_cast<const uint64_t*>(src) + (size_t)first * words;
  for (int w = tid; w < nb * words; w += threads) dst[w] = g[w];
}

// every layout: byte offsets of its sections from smem (what each holds is said where it is taken), and their end
struct LdsLayout {
  uint32_t end = 0;
  __host__ __device__ constexpr uint32_t bytes() const { return end; }
};

// ---- resolve_round<PF, QUOTA> --------------------------------------------------------------------------------------
// `shape`: the profile scores RequestedToCapacityRatio (PF_FIT_RTCR) and the kernel keeps the shape table in LDS
struct ResolveLds : LdsLayout {
  uint32_t cand, pods, par, hash, prevn, bitmap, lut;
};
__host__ __device__ constexpr ResolveLds resolve_lds(int nb, int bitmap_words, bool shape = false) {
  LdsCarver c;
  ResolveLds L{};
  L.cand = c.take<uint64_t, 16>(nb * kCandStride);  // [nb][kCandStride] the pods' records (LDS-DMA)
  L.pods = c.take<DevPod, 16>(nb);                  // [nb] DevPod (LDS-DMA)
  L.par = c.take<uint64_t>(kParWords);              // EvalParams (rare-path copy)
  L.hash = c.take<uint32_t, 16>(kModHash);          // node → slot (uint4 clears)
  L.prevn = c.take<uint32_t>(kMaxMod);              // earlier rounds' nodes
  L.bitmap = c.take<uint32_t, 16>(bitmap_words);    // modified rows (uint4 clears)
  // lut[0..100] as uint8_t, zero-padded (only with `shape`).  Bytes, not words: 101 bytes span 26 dwords, fewer than
  // the 64 banks, so two lanes on one bank read the same dword and a per-lane byte lookup cannot conflict
  L.lut = c.take<uint8_t, 16>(shape ? kFitLutBytes : 0);
  L.end = c.bytes();
  return L;
}

// ---- resolve_round_numa, resolve_round_numa2 -----------------------------------------------------------------------
constexpr int kNumaPre = 2;  // candidates per pod whose rows resolve_round_numa2's prologue reads into LDS
constexpr int kPreWords = kRowWords + kNumaStaticWords + kNumaMutWords + kViewWords;
struct NumaSlotsLds {  // what both NUMA resolvers start with
  uint32_t cand, pods, npods, ns, nm;
};
__host__ __device__ constexpr NumaSlotsLds numa_slots_lds(LdsCarver& c, int nb) {
  NumaSlotsLds S{};
  S.cand = c.take<uint64_t>(nb * kCandStride);  // [nb][kCandStride]
  S.pods = c.take<DevPod>(nb);
  S.npods = c.take<NumaPod>(nb);
  S.ns = c.take<NumaStatic>(kWave);  // of the modified rows (slots)
  S.nm = c.take<NumaMut>(kWave);     // of the slots (committed)
  return S;
}
struct NumaLds : LdsLayout {
  NumaSlotsLds s;
  uint32_t prevn, bitmap;
};
__host__ __device__ constexpr NumaLds numa_lds(int nb, int bitmap_words) {
  LdsCarver c;
  NumaLds L{};
  L.s = numa_slots_lds(c, nb);
  L.prevn = c.take<uint32_t>(kWave);  // earlier rounds' winners
  L.bitmap = c.take<uint32_t>(bitmap_words);
  L.end = c.bytes();
  return L;
}
struct Numa2Lds : LdsLayout {
  NumaSlotsLds s;
  uint32_t row, view, rnm, key, aff, misc, ver, node, c, bitmap, prevn, pre;
};
__host__ __device__ constexpr Numa2Lds numa2_lds(int nb, int bitmap_words, int npre) {
  LdsCarver c;
  Numa2Lds L{};
  L.s = numa_slots_lds(c, nb);
  L.row = c.take<Row>(kWave);            // of the slots (committed)
  L.view = c.take<NumaView>(kWave);      // of each slot's current state
  L.rnm = c.take<NumaMut>(1);            // the reserver's, after its Reserve
  L.key = c.take<uint64_t>(kWave);       // the scorer's keys of the current pod
  L.aff = c.take<uint64_t>(kWave * 2);   // the scorer's affinities (NumaHint)
  L.misc = c.take<uint64_t>(4);          // 0 = the current pod's e key (0 = none)
  L.ver = c.take<uint32_t>(kWave);       // slot state versions
  L.node = c.take<uint32_t>(kWave);      // node of each slot
  L.c = c.take<int32_t>(16);             // 0 nM, 1 stop, 4 timed out, 5 abort
  L.bitmap = c.take<uint32_t>(bitmap_words);
  L.prevn = c.take<uint32_t>(kWave);     // earlier rounds' winners (prologue)
  L.pre = c.take<uint64_t>(nb * npre * kPreWords);  // [nb][npre] Row, NumaStatic, NumaMut, NumaView (npre: 0 or kNumaPre)
  L.end = c.bytes();
  return L;
}

// ---- resolve_round_ds ----------------------------------------------------------------------------------------------
struct DsLds : LdsLayout {
  uint32_t cand, pods, dpods, cur, stg, q, qdev, srow, d0, r0, bitmap;
};
__host__ __device__ constexpr DsLds ds_lds(int nb, int nq, bool sharded, int bitmap_words) {
  LdsCarver c;
  DsLds L{};
  L.cand = c.take<uint64_t>(nb * kCandStride);  // [nb][kCandStride]
  L.pods = c.take<DevPod>(nb);
  L.dpods = c.take<DsPod>(nb);
  L.cur = c.take<DsNode>(kWave);                // of the modified rows, current
  L.stg = c.take<DsNode>(nb);                   // of each pod's top candidate
  L.q = c.take<QuotaRow>(nq);
  L.qdev = c.take<int64_t>(nb * kQuotaRes);     // the pods' device quota requests
  L.srow = c.take<Row>(nb);                     // of each pod's top candidate
  L.d0 = c.take<DsNode>(sharded ? kWave : 0);   // round-start DsNode per modified lane
  L.r0 = c.take<Row>(sharded ? kWave : 0);      // round-start Row
  L.bitmap = c.take<uint32_t>(bitmap_words);
  L.end = c.bytes();
  return L;
}

// ---- xr_resolve<XF> (xr_dev.h) -------------------------------------------------------------------------------------
// Exact-round features (compile-time: the kernels carry only the plugins the profile enables, so the Fit /
// LoadAware / Reservation-only variants keep their registers, and none spills for code it never runs)
constexpr int XF_NUMA = 1, XF_DS = 2, XF_DEF = 4;
struct XrLds : LdsLayout {
  uint32_t cand, pods, rpods, dpods, npods, defp, aux, q, qdev, bitmap;
};
__host__ __device__ constexpr XrLds xr_lds(int xf, int nq, bool aux, int bitmap_words) {
  LdsCarver c;
  XrLds L{};
  L.cand = c.take<uint64_t>(kXrPods * (kC + 1));  // [kXrPods][kC + 1] keys and ub
  L.pods = c.take<DevPod>(kXrPods);
  L.rpods = c.take<RsvPod>(kXrPods);
  L.dpods = c.take<DsPod>((xf & XF_DS) ? kXrPods : 0);
  L.npods = c.take<NumaPod>((xf & XF_NUMA) ? kXrPods : 0);
  L.defp = c.take<uint64_t>((xf & XF_DEF) ? kXrPods * kDefPodWords : 0);  // DefPod, kDefPodWords apart
  L.aux = c.take<int64_t>(aux ? kXrPods * kAux : 0);  // aux requests (staged when the queue carries any)
  L.q = c.take<QuotaRow>(nq);
  L.qdev = c.take<int64_t>(nq > 0 ? kXrPods * kQuotaRes : 0);
  L.bitmap = c.take<uint32_t>(bitmap_words);
  L.end = c.bytes();
  return L;
}

// ---- eval_round ----------------------------------------------------------------------------------------------------
// A block of ew waves (tiles of tile_nodes nodes) × ppw pods.  On tile groups (`combine`) each wave stages its pods'
// values of its tile, ew · ppw · tile_nodes uint32 as [pod][tile][lane][j] — a wave's stores and the selecting wave's
// loads both run over consecutive lanes, so neither meets a bank conflict — and each wave has rg words for the keys it
// selected.  4 KiB per pod at the 1,024-node group: 32 KiB at ppw = 8, two blocks per CU resident as the kernel's four
// waves per SIMD allow.  A block whose staging would pass kEvalStageCap (ppw > 15 there) does not stage: two blocks
// would no longer share a CU's 160 KiB, and the launch would need the large-LDS opt-in; such a pod group, and a shard without tile groups,
// parks tile lists instead: [ew][ppw·kR] uint64, ppw lists of kR keys per wave (the stride the kernel indexes with).
constexpr uint32_t kEvalStageCap = 64 * 1024;
struct EvalLds : LdsLayout {
  uint32_t lists, vals, sel, lut;
  bool staged;  // the values are staged and selected per (pod, tile group); else tile lists (combined if `combine`)
};
__host__ __device__ constexpr EvalLds eval_lds(int ew, int tile_nodes, int rg, int ppw, bool combine,
                                               bool shape = false) {
  LdsCarver c;
  EvalLds L{};
  const uint32_t vals = (uint32_t)ew * (uint32_t)ppw * (uint32_t)tile_nodes;
  L.staged = combine && vals * 4u + (uint32_t)(ew * rg) * 8u <= kEvalStageCap;
  if (L.staged) {
    L.vals = L.lists = c.take<uint32_t, 16>(vals);  // [ppw][ew][kWave][tile_nodes / kWave]
    L.sel = c.take<uint64_t, 16>(ew * rg);          // [ew][rg] selected keys, before their ranking
  } else {
    L.lists = c.take<uint64_t, 16>(ew * ppw * kR);  // [ew][ppw][kR]
  }
  // the RequestedToCapacityRatio shape table (only with `shape`, PF_FIT_RTCR; as resolve_lds's): after the staging
  // decision, which therefore is the same with and without it
  L.lut = c.take<uint8_t, 16>(shape ? kFitLutBytes : 0);
  L.end = c.bytes();
  return L;
}

// ---- the bounds at the engine's maxima -----------------------------------------------------------------------------
// kMaxNodes / 32 bitmap words: 64 KiB; kMaxB records: 64 KiB.  These resolvers fit whatever the configuration, so
// prepare_rounds' / run_xr's check against kMaxLds never refuses them.  Two do not fit at their maxima, and there the
// run-time check is the bound: resolve_round_ds (kMaxDsB pods, KG_MAX_QUOTAS quotas, several ranks, kMaxNodes nodes:
// 177,920 B), which prepare_rounds refuses, and resolve_round_numa2, which launch_resolve replaces by the one-wave
// resolve_round_numa where it does not fit.
constexpr int kMaxBitmapWords = (int)(kMaxNodes / 32);
static_assert(resolve_lds(kMaxB, kMaxBitmapWords).bytes() <= kMaxLds, "resolve_round at kMaxB pods, kMaxNodes nodes");
// eval_round at its shape (8 waves of 128-node tiles, 8 keys per group list): two blocks of 8 pods per wave share a CU
// with their values staged; past kEvalStageCap a block parks tile lists, which fit the default dynamic-LDS limit at
// any pod count
static_assert(eval_lds(8, 128, 8, 8, true).staged && 2 * eval_lds(8, 128, 8, 8, true).bytes() <= kMaxLds,
              "eval_round: two blocks per CU at 8 pods per wave");
static_assert(eval_lds(8, 128, 8, 15, true).staged && eval_lds(8, 128, 8, 15, true).bytes() <= kEvalStageCap &&
                  !eval_lds(8, 128, 8, 16, true).staged && eval_lds(8, 128, 8, kMaxB, true).bytes() <= kEvalStageCap &&
                  eval_lds(8, 128, 8, kMaxB, false).bytes() <= kEvalStageCap,
              "eval_round: staged up to 15 pods per wave, tile lists beyond, 64 KiB at most either way");
static_assert(resolve_lds(kMaxB, kMaxBitmapWords, true).bytes() <= kMaxLds &&
                  2 * eval_lds(8, 128, 8, 8, true, true).bytes() <= kMaxLds &&
                  eval_lds(8, 128, 8, 15, true, true).bytes() <= kEvalStageCap &&
                  eval_lds(8, 128, 8, kMaxB, true, true).bytes() <= kEvalStageCap &&
                  eval_lds(8, 128, 8, kMaxB, false, true).bytes() <= kEvalStageCap,
              "the same bounds with the RequestedToCapacityRatio shape table");
static_assert(numa_lds(kMaxB, kMaxBitmapWords).bytes() <= kMaxLds, "resolve_round_numa at kMaxB pods, kMaxNodes nodes");
static_assert(xr_lds(XF_NUMA | XF_DS | XF_DEF, KG_MAX_QUOTAS, true, kMaxBitmapWords).bytes() <= kMaxLds,
              "xr_resolve with every section at kMaxNodes nodes");

}  // namespace kg
