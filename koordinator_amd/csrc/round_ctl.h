// The round engine's control protocol: the words of the two device control blocks, by name, and the steps every
// resolver takes on the chain (wait for the predecessor, abort when the round is stale, read the earlier rounds'
// modified-row lists, write its own, advance the cursor, publish).  DESIGN.md §3.3 / §3.4 describe the protocol;
// this header is its definition.  Included by engine.hip and rsv_dev.h; xr_dev.h is compiled inside engine.hip and
// sees it from there.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace kg {

// kg_engine::cursor: the round engine's control block, CTL_WORDS int64 words, written by the resolvers and read by
// the host after every batch of rounds.
enum CtlWord : int {
  CTL_CURSOR = 0,        // first pod no round has consumed yet
  CTL_ROUNDS = 1,        // rounds run in this schedule call
  CTL_CONSUMED = 2,      // pods consumed in this schedule call
  CTL_POISON = 3,        // an int32 in the word's low half: a round stopped early, the rest of its batch is skipped
  CTL_SEQ = 4,           // sequence number of the last resolver that published
  CTL_ERROR = 5,         // device error: a resolver's chain wait timed out
  CTL_SLOW = 6,          // diagnostics: pods re-scored on the chain
  CTL_RESERVED_7 = 7,    // unused: no kernel writes it, and the words after it keep their indices
  CTL_ACTIVE_TICKS = 8,  // resolvers' active time, s_memrealtime ticks
  CTL_WORDS = 16
};
// run_batch clears poison, sequence and error with one memset
static_assert(CTL_SEQ == CTL_POISON + 1 && CTL_ERROR == CTL_SEQ + 1, "poison, sequence and error words are adjacent");

// kg_engine::rsv_ws: the exact pass's and the exact rounds' workspace, WS_WORDS unsigned 64-bit words.
enum WsWord : int {
  WS_QUOTA_TAG = 0,  // per-pod pass: the pod whose predecessor's quota charge rsv_select still has to write
  WS_NOM_KILL = 1,   // per-pod pass with nominated pods: 1 + the table entry of the call's last pod, 0 = it has none
  WS_CURSOR = 3,     // next pod of the call (word 2 is unused)
  WS_END = 4,        // the call's end (kernels launched from a graph read it here)
  WS_ROUNDS = 5,     // exact rounds run in this call
  WS_CONSUMED = 6,   // pods those rounds consumed
  WS_ZERO = 7,       // always 0: what merge_round reads as poison in the exact rounds, which never poison
  WS_WORDS = 8
};

constexpr int kMaxB = 64;             // pods per round: modified rows are held one per lane of the resolver wave
constexpr int kMaxDepth = 4;          // pipelined rounds in flight (streams)
constexpr int kMaxMod = 2 * kWave;    // modified-row slots: two register banks
constexpr int kModHash = 512;         // node → slot hash for de-duplicating earlier rounds' lists
constexpr int kModListStride = 1 + kMaxB;  // [count, node ids...] per round slot
// chain_wait gives up after this many polls with s_sleep(1) between them (seconds): a resolver whose predecessor
// never publishes reports CTL_ERROR instead of hanging the device
constexpr int64_t kSpinLimit = 1 << 25;

__device__ __forceinline__ uint32_t mod_hash(uint32_t node) { return (node * 2654435761u) >> (32 - 9); }
static_assert(kModHash == 512, "hash width");

// insert node → slot; returns the slot already holding node when present
__device__ __forceinline__ int mod_insert(uint32_t* h, uint32_t node, int slot) {
  const uint32_t v = ((node + 1u) << 8) | (uint32_t)slot;
  uint32_t i = mod_hash(node);
  for (int it = 0; it < kModHash; ++it) {
    const uint32_t prev = atomicCAS(&h[i], 0u, v);
    if (prev == 0u) return slot;
    if ((prev >> 8) == node + 1u) return (int)(prev & 0xFFu);
    i = (i + 1u) & (kModHash - 1);
  }
  return -1;
}

// End of a resolver: every store of this wave visible device-wide, then CTL_SEQ = seq (agent-scope release) for
// the next round's resolver, which may already be resident on another round stream.
// (r5) Release only (the guide's producer form): this wave's stores drained, the XCD L2 written back, the wait after
// the write-back kept by inline asm (the compiler may drop it), then a relaxed flag store.  The acq_rel
// __threadfence() it replaces also invalidated the L2 — a cost on the serial chain that nothing after it needs.
__device__ __forceinline__ void publish_round(int64_t* ctl, int64_t seq) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (threadIdx.x == 0) __hip_atomic_store(&ctl[CTL_SEQ], seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Start of a resolver's chained part: the calling thread waits until the previous round's resolver (another round
// stream) has published, i.e. CTL_SEQ ≥ seq − 1; `wait` = 0 for a batch's first round, which has no predecessor.
// Returns 1 when it gave up (kSpinLimit).  One thread calls it and the kernel broadcasts the result; the agent-scope
// acquire fence that makes the predecessor's rows, cursor, poison and list visible to the other threads follows at
// the call site.
__device__ __forceinline__ int chain_wait(const int64_t* ctl, int64_t seq, int wait) {
  if (!wait) return 0;
  int64_t it = 0;
  while (__hip_atomic_load(&ctl[CTL_SEQ], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < seq - 1) {
    __builtin_amdgcn_s_sleep(1);
    if (++it > kSpinLimit) return 1;
  }
  return 0;
}

// the round must not run: no predecessor, an earlier round of the batch stopped early, or the cursor moved
__device__ __forceinline__ bool round_stale(const int64_t* ctl, const int32_t* poison, int64_t first, int timed_out) {
  return timed_out || *poison || ctl[CTL_CURSOR] != first;
}

// a stale round retires: the timeout is reported, and the successor still finds its sequence number
__device__ __forceinline__ void round_abort(int64_t* ctl, int64_t seq, int timed_out) {
  if (threadIdx.x == 0 && timed_out) ctl[CTL_ERROR] = 1;
  publish_round(ctl, seq);
}

// the list of the d-th round before round slot `slot` (round r uses slot r % depth)
__device__ __forceinline__ const int32_t* prev_list(const int32_t* modlists, int slot, int d, int depth) {
  return modlists + (size_t)(((slot - d) % depth + depth) % depth) * kModListStride;
}

// The n_prev earlier rounds' lists concatenated into s_prevn (duplicates included) by the lanes of one wave; returns
// their total length.  `active` = false: the thread only counts (resolve_round_numa2's second wave).
__device__ __forceinline__ int gather_prev_lists(const int32_t* modlists, int slot, int depth, int n_prev,
                                                 uint32_t* s_prevn, int lane, bool active) {
  int n = 0;
  for (int d = 1; d <= n_prev; ++d) {
    const int32_t* ml = prev_list(modlists, slot, d, depth);
    const int c = ml[0];
    if (active)
      for (int t = lane; t < c; t += kWave) s_prevn[n + t] = (uint32_t)ml[1 + t];
    n += c;
  }
  return n;
}

// The NUMA resolvers' de-duplication of the n ≤ kWave gathered nodes (n is what gather_prev_lists returned): one
// node per lane of the active wave, a node met earlier in the list dropped by a readlane compare, the survivors
// compacted to s_prevn[0, count) in list order.  Every thread of the workgroup calls it (it holds the barriers
// around the LDS reads and writes); returns the count on the active wave, 0 on the others.
__device__ __forceinline__ int compact_prev_nodes(uint32_t* s_prevn, int n, int lane, bool active) {
  __syncthreads();
  const uint32_t node = (active && lane < n) ? s_prevn[lane] : 0xFFFFFFFFu;
  bool dup = false;
  if (active)
    for (int k = 0; k < n; ++k) dup |= lane > k && node == (uint32_t)__builtin_amdgcn_readlane((int)node, k);
  const bool keep = active && lane < n && !dup;
  const uint64_t km = __ballot(keep);
  const uint64_t lane_lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  __syncthreads();
  if (keep) s_prevn[__popcll(km & lane_lt)] = node;
  __syncthreads();
  return __popcll(km);
}

// This round's list for the next rounds: lane l's pod was placed on `node` when `mine` (duplicates allowed: the
// readers keep one slot per node).  Called by every lane of one wave.
__device__ __forceinline__ void publish_mod_list(int32_t* modlists, int slot, bool mine, uint32_t node, int lane) {
  int32_t* my_mod = modlists + (size_t)slot * kModListStride;
  const uint64_t lane_lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  const uint64_t bm = __ballot(mine);
  if (mine) my_mod[1 + __popcll(bm & lane_lt)] = (int32_t)node;
  if (lane == 0) my_mod[0] = __popcll(bm);
}

// The round's bookkeeping, on one lane, before publish_round: the cursor past the pods consumed, the call's totals,
// poison when the round stopped early (POISONS = false: cursor-driven rounds, which just restart at the cursor), and
// the active time since t_active.
template <bool POISONS = true>
__device__ __forceinline__ void round_close(int64_t* ctl, int32_t* poison, int64_t first, int consumed, int nb,
                                            uint64_t t_active) {
  ctl[CTL_CURSOR] = first + consumed;
  ctl[CTL_ROUNDS] += 1;
  ctl[CTL_CONSUMED] += consumed;
  if (POISONS && consumed < nb) *poison = 1;
  ctl[CTL_ACTIVE_TICKS] += (int64_t)(__builtin_amdgcn_s_memrealtime() - t_active);
}

}  // namespace kg
