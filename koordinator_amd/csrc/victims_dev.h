// kg_node_bound_pods_set / kg_pods_select_victims_resident / kg_pods_preempt_resident (added within ABI 18): the bound
// pods preemption reads, resident in HBM, and SelectVictimsOnNode's per-node front half on the device — the canPreempt
// selection, the MoreImportantPod order and the filterPodsWithPDBViolation split (koordinator
// elasticquota/preempt.go:139-170, 222-267, 283-294; pkg/scheduler/util MoreImportantPod restated as published,
// parity-unpinned) — feeding the unchanged select_victims and pick_* kernels.
//
// The table is a slab of entries, one array per field (BpCols), and a directory entry {off, len, cap} per node slot.
// Every list is stored in MoreImportantPod order (priority descending, earlier start first, ties in the caller's
// order: the host sorts at set time), so a call never sorts: a subset of a sorted list is sorted.
//
// Plain launches on the engine stream, in stream order (no spin on another kernel, no cooperative launch,
// no atomics):
//   bp_scatter   set time: one wavefront per replaced list copies it from the staging arrays to its place in the slab
//                and writes the node's directory entry.
//   rv_select    one wavefront per candidate, 64 entries a step.  The rule test of a step is one ballot.  Lane b holds
//                the remaining budget of PDB b (a fresh copy of pdb_allowed per candidate); the walk over the set bits
//                of the ballot broadcasts each potential victim's PDB mask, every matching lane decrements, and the
//                entry is violating when the ballot of "bit b set and counter < 0" is non-zero.  Writes a byte per
//                entry (bit 0 potential, bit 1 violating) and the candidate's two counts.
//   rv_scan      one block: the exclusive scan of the potential counts over the candidates (each thread a contiguous
//                chunk of ⌈n / 1024⌉ candidates, wave scans by shuffles, the waves through LDS) = select_victims' offsets.
//   rv_compact   one wavefront per candidate writes the call's arrays at its offset: the violating entries first, then
//                the others, each group in list order (ballot + prefix population count) — the Victim record, the
//                violating flag, the priority, the start, and the slab position it came from.
//   rv_winner    after pick_final: the winner's victim positions → (uid, caller-list index), behind the pick header.
//   rv_export    the unfused form's per-entry byte and rank, in the caller's list order.
// Included by engine.hip after pick_dev.h.
#pragma once

constexpr int kRvThreads = 256;  // 4 waves per block, one candidate (or list) per wave
constexpr int kRvWaves = kRvThreads / kWave;
constexpr int kRvScanThreads = 1024;
constexpr int kVictimWords = (int)(sizeof(Victim) / 8);
static_assert(sizeof(Victim) % 8 == 0, "Victim is copied as 8-byte words");

struct BpDir {
  int64_t off;  // first entry of the node's list in the slab
  int32_t len;  // entries in use
  int32_t cap;  // entries reserved at off
};
static_assert(sizeof(BpDir) == 16, "BpDir layout");

// the slab's (or the staging area's) arrays: the dry-run record, then the selection fields one array each
struct BpCols {
  Victim* vic;
  int32_t* prio;    // PodPriority
  int64_t* start;   // GetPodStartTime, unix nanoseconds
  int32_t* flags;   // kg_pod.flags & KG_POD_NON_PREEMPTIBLE
  int64_t* quota;   // kg_pod.quota_id
  uint64_t* mask;   // bit b: matches PDB b and is not in its DisruptedPods
  int64_t* uid;     // kg_pod.uid
  int32_t* cidx;    // index in the caller's list
};

// one replaced list of a kg_node_bound_pods_set call: `len` entries from staging position src to slab position dst
struct BpList {
  int64_t dst, src;
  int32_t node, len, cap, pad;
};
static_assert(sizeof(BpList) == 32, "BpList layout");

// the preemptor's side of the rule
struct RvCall {
  int64_t pod_quota;
  int32_t pod_priority;
  int32_t quota_rule;  // KG_PREEMPT_RULE_QUOTA
  int32_t n_pdbs;
  int32_t pad;
};

__device__ __forceinline__ uint64_t rv_bcast_u64(uint64_t v, int src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, kWave);
  const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, kWave);
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ int64_t rv_shfl_up_i64(int64_t v, int d) {
  const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)(uint64_t)v, d, kWave);
  const uint32_t hi = (uint32_t)__shfl_up((int)(uint32_t)((uint64_t)v >> 32), d, kWave);
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// canPreempt: upstream's rule (lower priority), or Koordinator's (also preemptible and of the preemptor's quota)
__device__ __forceinline__ bool rv_can_preempt(const RvCall& R, int32_t prio, int32_t flags, int64_t quota) {
  if (prio >= R.pod_priority) return false;
  if (!R.quota_rule) return true;
  return !(flags & KG_POD_NON_PREEMPTIBLE) && quota == R.pod_quota;
}

__global__ __launch_bounds__(kRvThreads) void bp_scatter(int64_t n_lists, const BpList* __restrict__ lists, BpCols S,
                                                         BpCols D, BpDir* __restrict__ dir) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t l = (int64_t)blockIdx.x * kRvWaves + threadIdx.x / kWave;  // uniform over the wave
  if (l >= n_lists) return;
  const BpList q = lists[l];
  for (int32_t k = lane; k < q.len; k += kWave) {
    const int64_t s = q.src + k, d = q.dst + k;
    D.prio[d] = S.prio[s];
    D.start[d] = S.start[s];
    D.flags[d] = S.flags[s];
    D.quota[d] = S.quota[s];
    D.mask[d] = S.mask[s];
    D.uid[d] = S.uid[s];
    D.cidx[d] = S.cidx[s];
  }
  const int64_t* sw = reinterpret_cast<const int64_t*>(S.vic + q.src);
  int64_t* dw = reinterpret_cast<int64_t*>(D.vic + q.dst);
  for (int64_t w = lane; w < (int64_t)q.len * kVictimWords; w += kWave) dw[w] = sw[w];
  if (lane == 0) dir[q.node] = BpDir{q.dst, q.len, q.cap};
}

// nodes == nullptr: candidate c is node slot c.  cnt[2c] = potential victims, cnt[2c + 1] = the PDB-violating ones.
__global__ __launch_bounds__(kRvThreads) void rv_select(BpCols B, const BpDir* __restrict__ dir, int64_t n_cand,
                                                        const int32_t* __restrict__ nodes, RvCall R,
                                                        const int32_t* __restrict__ pdb_allowed,
                                                        int32_t* __restrict__ out_nodes, int32_t* __restrict__ cnt,
                                                        uint8_t* __restrict__ eflag) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t c = (int64_t)blockIdx.x * kRvWaves + threadIdx.x / kWave;  // uniform over the wave
  if (c >= n_cand) return;
  const int32_t node = nodes ? nodes[c] : (int32_t)c;
  const BpDir d = dir[node];
  const uint64_t pdbs = R.n_pdbs >= 64 ? ~0ull : (1ull << R.n_pdbs) - 1;
  int32_t counter = lane < R.n_pdbs ? pdb_allowed[lane] : 0;  // pdbsAllowed[lane], fresh for this node
  int32_t npot = 0, nvio = 0;
  for (int32_t base = 0; base < d.len; base += kWave) {  // uniform: ⌈len / 64⌉ steps
    const bool in = base + lane < d.len;
    const int64_t at = d.off + base + lane;
    bool pot = false;
    uint64_t m = 0;
    if (in) {
      pot = rv_can_preempt(R, B.prio[at], B.flags[at], B.quota[at]);
      m = pot ? B.mask[at] & pdbs : 0;
    }
    const uint64_t pb = __builtin_amdgcn_ballot_w64(pot);
    uint64_t walk = __builtin_amdgcn_ballot_w64(m != 0);  // the potential victims that match a PDB, in list order
    uint64_t vb = 0;
    while (walk) {  // uniform
      const int j = __builtin_ctzll(walk);
      walk &= walk - 1;
      const bool hit = (rv_bcast_u64(m, j) >> lane) & 1;
      if (hit) --counter;
      if (__builtin_amdgcn_ballot_w64(hit && counter < 0)) vb |= 1ull << j;
    }
    if (in) eflag[at] = (uint8_t)((pot ? 1 : 0) | ((vb >> lane) & 1 ? 2 : 0));
    npot += __popcll(pb);
    nvio += __popcll(vb);
  }
  if (lane == 0) {
    out_nodes[c] = node;
    cnt[2 * c] = npot;
    cnt[2 * c + 1] = nvio;
  }
}

// off[c] = the potential victims of the candidates before c; off[n_cand] = all of them
__global__ __launch_bounds__(kRvScanThreads) void rv_scan(const int32_t* __restrict__ cnt, int64_t n_cand,
                                                          int64_t* __restrict__ off) {
  __shared__ int64_t s_wave[kRvScanThreads / kWave];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int64_t chunk = (n_cand + kRvScanThreads - 1) / kRvScanThreads;
  const int64_t t0 = (int64_t)threadIdx.x * chunk;
  const int64_t c0 = t0 < n_cand ? t0 : n_cand, c1 = c0 + chunk < n_cand ? c0 + chunk : n_cand;
  int64_t sum = 0;
  for (int64_t c = c0; c < c1; ++c) sum += cnt[2 * c];
  int64_t inc = sum;  // inclusive scan over the wave
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const int64_t t = rv_shfl_up_i64(inc, d);
    if (lane >= d) inc += t;
  }
  if (lane == kWave - 1) s_wave[wave] = inc;
  __syncthreads();
  int64_t run = inc - sum;
  for (int w = 0; w < wave; ++w) run += s_wave[w];
  for (int64_t c = c0; c < c1; ++c) {
    off[c] = run;
    run += cnt[2 * c];
  }
  if (threadIdx.x == kRvScanThreads - 1) off[n_cand] = run;  // the last thread's chunk ends the candidates
}

// the call's arrays, per candidate the violating entries first, then the others, each group in list order.
// erank (nullable, indexed like eflag by slab position): the entry's rank in that order, -1 = not a potential victim.
__global__ __launch_bounds__(kRvThreads) void rv_compact(BpCols B, const BpDir* __restrict__ dir, int64_t n_cand,
                                                         const int32_t* __restrict__ nodes,
                                                         const int32_t* __restrict__ cnt, const int64_t* __restrict__ off,
                                                         const uint8_t* __restrict__ eflag, Victim* __restrict__ vic,
                                                         uint8_t* __restrict__ viol, int32_t* __restrict__ prio,
                                                         int64_t* __restrict__ start, int32_t* __restrict__ src,
                                                         int32_t* __restrict__ erank) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t c = (int64_t)blockIdx.x * kRvWaves + threadIdx.x / kWave;  // uniform over the wave
  if (c >= n_cand) return;
  const BpDir d = dir[nodes[c]];
  const int64_t o = off[c];
  const int32_t first_other = cnt[2 * c + 1];
  const uint64_t below = (1ull << lane) - 1;
  int32_t wv = 0, wn = 0;  // written so far of either group (uniform)
  for (int32_t base = 0; base < d.len; base += kWave) {
    const bool in = base + lane < d.len;
    const int64_t at = d.off + base + lane;
    const uint8_t f = in ? eflag[at] : 0;
    const bool isv = (f & 3) == 3, isn = (f & 3) == 1;
    const uint64_t vb = __builtin_amdgcn_ballot_w64(isv), nb = __builtin_amdgcn_ballot_w64(isn);
    const int32_t rank = isv ? wv + __popcll(vb & below) : isn ? first_other + wn + __popcll(nb & below) : -1;
    if (rank >= 0) {
      const int64_t p = o + rank;
      vic[p] = B.vic[at];
      viol[p] = isv ? 1 : 0;
      prio[p] = B.prio[at];
      start[p] = B.start[at];
      src[p] = (int32_t)at;
    }
    if (erank && in) erank[at] = rank;
    wv += __popcll(vb);
    wn += __popcll(nb);
  }
}

// the winner's victims (pick_final's positions into the call's arrays) as (uid, caller-list index)
__global__ __launch_bounds__(kRvThreads) void rv_winner(const kg_preempt_pick* __restrict__ hdr,
                                                        const int32_t* __restrict__ pos, const int32_t* __restrict__ src,
                                                        BpCols B, int64_t cap, int64_t* __restrict__ out_uid,
                                                        int32_t* __restrict__ out_cidx) {
  const int64_t n = hdr->n_victims < cap ? hdr->n_victims : cap;
  for (int64_t k = threadIdx.x; k < n; k += kRvThreads) {
    const int32_t s = src[pos[k]];
    out_uid[k] = B.uid[s];
    out_cidx[k] = B.cidx[s];
  }
}

// the unfused form: per resident entry of the candidates, at ebase[c] + its caller-list index, the byte (bit 0
// potential victim, bit 1 PDB-violating, bit 2 kept as victim) and its rank in reprieve order
__global__ __launch_bounds__(kRvThreads) void rv_export(BpCols B, const BpDir* __restrict__ dir, int64_t n_cand,
                                                        const int32_t* __restrict__ nodes, const int64_t* __restrict__ off,
                                                        const int64_t* __restrict__ ebase,
                                                        const uint8_t* __restrict__ eflag,
                                                        const int32_t* __restrict__ erank,
                                                        const uint8_t* __restrict__ kept, uint8_t* __restrict__ out_flag,
                                                        int32_t* __restrict__ out_rank) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t c = (int64_t)blockIdx.x * kRvWaves + threadIdx.x / kWave;
  if (c >= n_cand) return;
  const BpDir d = dir[nodes[c]];
  for (int32_t k = lane; k < d.len; k += kWave) {
    const int64_t at = d.off + k;
    const int32_t r = erank[at];
    const int64_t to = ebase[c] + B.cidx[at];
    out_flag[to] = (uint8_t)(eflag[at] | (r >= 0 && kept[off[c] + r] ? 4 : 0));
    out_rank[to] = r;
  }
}
