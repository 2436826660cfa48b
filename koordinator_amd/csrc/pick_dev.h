// kg_pods_pick_candidate / kg_pods_preempt (added within ABI 18): the preemption evaluator's SelectCandidate →
// pickOneNodeForPreemption reduced on the device — one kg_preempt_pick and the winner's victim positions instead of a
// status word and a violating count per candidate and a byte per potential victim copied to the host.
//
// The rule (k8s.io/kubernetes v1.24 pkg/scheduler/framework/preemption/preemption.go pickOneNodeForPreemption and
// pkg/scheduler/util GetEarliestPodStartTime, restated as published; parity-unpinned).  Among the
// candidates whose dry-run status is 0, with victims = the kept entries of the candidate's segment in list order:
//   0. a candidate without victims wins at once;     3. lowest sum of int64(priority) + 2^31;
//   1. fewest PDB violations;                         4. fewest victims;
//   2. lowest priority of the FIRST victim;           5. latest "earliest start among the victims at the list's maximum
//                                                        priority";   6. lowest candidate position.
// Each step narrows what the one before left, so the winner is the minimum of a 256-bit key (PickKey) whose fields are
// those criteria from the most significant bit down, the position last: the key is unique per candidate, the minimum
// does not depend on how the candidates are split over lanes, waves and blocks.
//
// Three plain launches on the engine stream, in stream order (no spin on another kernel, no cooperative
// launch, no atomics on the result), over scratch of their own (the engine's pick_buf):
//   pick_keys    one wavefront per candidate, the lanes striding its victim segment 64 entries a step (coalesced reads
//                of kept / priority / start).  Per step one ballot of "kept": its find-first in the first non-empty
//                step is Victims.Pods[0], its population count adds to the victim count.  Each lane keeps its own sum
//                and (maximum priority, earliest start at that priority); after the loop a wave sum, a wave max of the
//                priority and a wave min of the start over the lanes at that maximum.  Lane 0 stores key[c].
//   pick_reduce  a fixed grid of blocks strides the keys; each thread keeps a running minimum, the waves combine by
//                shuffles and the block through LDS.  One partial (key, eligible count) per block.
//   pick_final   one block reduces the partials, writes the kg_preempt_pick header and, behind it, the winner's kept
//                positions in list order (one wave: ballot + prefix population count per 64 entries), so the host makes a
//                single device-to-host copy.
// Included by engine.hip after diag_dev.h.
#pragma once

constexpr int kPickThreads = 256;                      // 4 waves per block
constexpr int kPickWaves = kPickThreads / kWave;
constexpr int kPickBlocks = 256;                       // pick_reduce's grid bound = pick_final's partials (one per thread)
constexpr uint32_t kPickNone = 0xFFFFFFFFu;            // position field of the key no eligible candidate has

// smaller wins; compared word by word from w[0].  Bits, most significant first:
//   w[0]  has victims (1) | numViolatingVictim (31) | priority of the first victim + 2^31 (32)
//   w[1]  sum over the victims of priority + 2^31 (< 2^63)
//   w[2]  victim count (32) | high half of E          E = ~(earliest start + 2^63): the latest start is the smallest E
//   w[3]  low half of E (32) | candidate position (32)
// An ineligible candidate is all ones; a candidate without victims is all zeros but for its position.
struct PickKey {
  uint64_t w[4];
};
struct PickPart {
  PickKey key;
  uint64_t eligible;
};

__host__ __device__ __forceinline__ bool pick_less(const PickKey& a, const PickKey& b) {
  if (a.w[0] != b.w[0]) return a.w[0] < b.w[0];
  if (a.w[1] != b.w[1]) return a.w[1] < b.w[1];
  if (a.w[2] != b.w[2]) return a.w[2] < b.w[2];
  return a.w[3] < b.w[3];
}
__device__ __forceinline__ PickKey pick_none() { return PickKey{{~0ull, ~0ull, ~0ull, ~0ull}}; }
__device__ __forceinline__ bool pick_eligible(const PickKey& k) { return (uint32_t)k.w[3] != kPickNone; }

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int m) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m, kWave);
  const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m, kWave);
  return ((uint64_t)hi << 32) | lo;
}
// butterfly reductions over the wave: every lane returns the result
__device__ __forceinline__ uint64_t pick_wave_sum(uint64_t v) {
#pragma unroll
  for (int m = kWave / 2; m > 0; m >>= 1) v += shfl_xor_u64(v, m);
  return v;
}
__device__ __forceinline__ uint64_t pick_wave_max(uint64_t v) {
#pragma unroll
  for (int m = kWave / 2; m > 0; m >>= 1) {
    const uint64_t o = shfl_xor_u64(v, m);
    v = o > v ? o : v;
  }
  return v;
}
__device__ __forceinline__ uint64_t pick_wave_min(uint64_t v) {
#pragma unroll
  for (int m = kWave / 2; m > 0; m >>= 1) {
    const uint64_t o = shfl_xor_u64(v, m);
    v = o < v ? o : v;
  }
  return v;
}
__device__ __forceinline__ PickKey pick_wave_min(PickKey k) {
#pragma unroll
  for (int m = kWave / 2; m > 0; m >>= 1) {
    PickKey o;
#pragma unroll
    for (int q = 0; q < 4; ++q) o.w[q] = shfl_xor_u64(k.w[q], m);
    if (pick_less(o, k)) k = o;
  }
  return k;
}

// key[c] of every candidate; `off`, `kept`, `prio`, `start` index the call's victims array
__global__ __launch_bounds__(kPickThreads) void pick_keys(int64_t n_cand, const int64_t* __restrict__ off,
                                                          const int32_t* __restrict__ reject,
                                                          const uint8_t* __restrict__ kept,
                                                          const int32_t* __restrict__ nvio,
                                                          const int32_t* __restrict__ prio,
                                                          const int64_t* __restrict__ start,
                                                          PickKey* __restrict__ key) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t c = (int64_t)blockIdx.x * kPickWaves + threadIdx.x / kWave;  // uniform over the wave
  if (c >= n_cand) return;
  if (reject[c] != 0) {
    if (lane == 0) key[c] = pick_none();
    return;
  }
  const int64_t k0 = off[c], k1 = off[c + 1];
  int64_t first = -1;
  uint32_t cnt = 0;
  uint64_t sum = 0;                      // this lane's share
  bool has = false;                      // this lane has seen a victim
  int32_t mx = 0;                        // its maximum priority and the earliest start at it
  int64_t ear = 0;
  for (int64_t base = k0; base < k1; base += kWave) {  // uniform: ⌈len / 64⌉ steps
    const int64_t k = base + lane;
    const bool v = k < k1 && kept[k] != 0;
    const uint64_t m = __builtin_amdgcn_ballot_w64(v);
    if (m == 0) continue;
    if (first < 0) first = base + __builtin_ctzll(m);
    cnt += (uint32_t)__popcll(m);
    if (v) {
      const int32_t p = prio[k];
      const int64_t s = start[k];
      sum += (uint64_t)((int64_t)p + (1ll << 31));
      if (!has || p > mx) {
        mx = p, ear = s, has = true;
      } else if (p == mx && s < ear) {
        ear = s;
      }
    }
  }
  PickKey out;
  if (cnt == 0) {
    out = PickKey{{0, 0, 0, (uint64_t)(uint32_t)c}};
  } else {
    sum = pick_wave_sum(sum);
    // lanes without a victim contribute 0 to the max; a lane with one contributes 2^32 + its biased priority
    const uint64_t lm = has ? (1ull << 32) | (uint32_t)((uint32_t)mx ^ 0x80000000u) : 0;
    const uint64_t gm = pick_wave_max(lm);
    const uint64_t le = (has && lm == gm) ? (uint64_t)ear ^ (1ull << 63) : ~0ull;  // biased: unsigned order = signed order
    const uint64_t E = ~pick_wave_min(le);
    const uint32_t p0 = (uint32_t)prio[first] ^ 0x80000000u;
    out.w[0] = 1ull << 63 | (uint64_t)((uint32_t)nvio[c] & 0x7FFFFFFFu) << 32 | p0;
    out.w[1] = sum;
    out.w[2] = (uint64_t)cnt << 32 | E >> 32;
    out.w[3] = E << 32 | (uint64_t)(uint32_t)c;
  }
  if (lane == 0) key[c] = out;
}

// part[b] = the minimum key over block b's share of the candidates and how many of them are eligible
__global__ __launch_bounds__(kPickThreads) void pick_reduce(const PickKey* __restrict__ key, int64_t n_cand,
                                                            PickPart* __restrict__ part) {
  __shared__ PickPart s_red[kPickWaves];
  PickKey best = pick_none();
  uint64_t elig = 0;
  for (int64_t c = (int64_t)blockIdx.x * kPickThreads + threadIdx.x; c < n_cand; c += (int64_t)gridDim.x * kPickThreads) {
    const PickKey k = key[c];
    elig += pick_eligible(k) ? 1 : 0;
    if (pick_less(k, best)) best = k;
  }
  best = pick_wave_min(best);
  elig = pick_wave_sum(elig);
  if ((threadIdx.x & (kWave - 1)) == 0) s_red[threadIdx.x / kWave] = PickPart{best, elig};
  __syncthreads();
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int w = 1; w < kPickWaves; ++w) {
    if (pick_less(s_red[w].key, best)) best = s_red[w].key;
    elig += s_red[w].eligible;
  }
  part[blockIdx.x] = PickPart{best, elig};
}

// the header and the winner's victim positions (≤ cap of them: the host checked cap against the longest segment)
__global__ __launch_bounds__(kPickThreads) void pick_final(const PickPart* __restrict__ part, int n_part,
                                                           const int32_t* __restrict__ nodes,
                                                           const int64_t* __restrict__ off,
                                                           const uint8_t* __restrict__ kept,
                                                           kg_preempt_pick* __restrict__ hdr,
                                                           int32_t* __restrict__ out_victims, int64_t cap) {
  __shared__ PickPart s_red[kPickWaves];
  PickKey best = pick_none();
  uint64_t elig = 0;
  if ((int)threadIdx.x < n_part) {  // n_part ≤ kPickBlocks = kPickThreads
    best = part[threadIdx.x].key;
    elig = part[threadIdx.x].eligible;
  }
  best = pick_wave_min(best);
  elig = pick_wave_sum(elig);
  if ((threadIdx.x & (kWave - 1)) == 0) s_red[threadIdx.x / kWave] = PickPart{best, elig};
  __syncthreads();
  if (threadIdx.x >= kWave) return;
  // wave 0, every lane: the block's result
#pragma unroll
  for (int w = 1; w < kPickWaves; ++w) {
    if (pick_less(s_red[w].key, best)) best = s_red[w].key;
    elig += s_red[w].eligible;
  }
  const int lane = threadIdx.x;
  kg_preempt_pick h{};
  h.candidate = -1;
  h.node_idx = -1;
  h.eligible = (int64_t)elig;
  if (!pick_eligible(best)) {
    if (lane == 0) *hdr = h;
    return;
  }
  const int64_t c = (int64_t)(uint32_t)best.w[3];
  h.candidate = c;
  h.node_idx = nodes[c];
  if (best.w[0] >> 63) {
    h.n_victims = (int64_t)(best.w[2] >> 32);
    h.num_violating = (int64_t)(best.w[0] >> 32 & 0x7FFFFFFFu);
    h.first_priority = (int64_t)(int32_t)((uint32_t)best.w[0] ^ 0x80000000u);
    h.sum_priorities = (int64_t)best.w[1];
    const uint64_t E = best.w[2] << 32 | best.w[3] >> 32;
    h.earliest_start_unix_nano = (int64_t)(~E ^ (1ull << 63));
  }
  if (lane == 0) *hdr = h;
  int64_t w = 0;  // written so far (uniform)
  for (int64_t base = off[c]; base < off[c + 1]; base += kWave) {
    const int64_t k = base + lane;
    const bool v = k < off[c + 1] && kept[k] != 0;
    const uint64_t m = __builtin_amdgcn_ballot_w64(v);
    const int64_t at = w + __popcll(m & ((1ull << lane) - 1));
    if (v && at < cap) out_victims[at] = (int32_t)k;
    w += __popcll(m);
  }
}
