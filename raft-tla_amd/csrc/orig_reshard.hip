// raftmc — recovering a raft_original checkpoint at another GPU count: the kernels.
// Included by orig_backend.hip inside namespace rmc; the host side is OrigGpu::reshard_load there,
// the index arithmetic reshard_plan.h.
//
// The source is W parts (the rank files of a multi-GPU checkpoint, or one single-GPU file), the
// target W' ranks.  Every target rank reads every level of the source in the canonical order
// (reshard_plan.h) in blocks of at most StateStore::kBlock states, and runs per block:
//   orig_reshard_classify  fingerprint of every state, its new owner (fp >> 32) mod W' as one byte, and
//                          the states per owner of every workgroup;
//   orig_reshard_scan      (one workgroup) an exclusive scan of those counts per owner, behind the
//                          level's running counts: every state's stable index among its owner's;
//   orig_reshard_place     the new id of every state into the level's map; the states this rank owns
//                          into its store, their parent pointers rewritten through the map of the
//                          level before.
// No rank exchanges anything: the maps are a function of the source and W' alone.  Only two maps
// are alive at a time (a parent lies in the level before its child).  W' = 1 fills the single-GPU
// store; it does not spill to the host, so a file that does not fit the device store ends as
// CAPACITY_OVERFLOW where a single-GPU file would have been spilled.

enum { OE_RESHARD_PARENT = 0x400 };   // a parent pointer that names no state of the level before

template <class S>
__global__ void __launch_bounds__(BS) orig_reshard_classify(const u32* states, u64 n, u64 seed, u32 world,
                                                            unsigned char* owner, u32* wg_count) {
  constexpr int NW = S::NW, NWP = (S::NW + 3) & ~3;
  __shared__ u32 wave_cnt[BS / 64][RESHARD_MAX_WORLD];
  const u64 i = (u64)blockIdx.x * BS + threadIdx.x;
  const int lane = __lane_id(), wave = threadIdx.x >> 6;
  u32 own = ~0u;
  if (i < n) {
    u32 w[NW];
#pragma unroll
    for (int q = 0; q < NW; ++q) w[q] = states[i * NWP + q];
    own = fp_owner(fp64(w, seed), world);
    owner[i] = (unsigned char)own;
  }
#pragma unroll
  for (u32 o = 0; o < (u32)RESHARD_MAX_WORLD; ++o) {
    const u32 c = (u32)__popcll(__ballot(own == o));
    if (lane == 0) wave_cnt[wave][o] = c;
  }
  __syncthreads();
  if (threadIdx.x < RESHARD_MAX_WORLD) {
    u32 c = 0;
#pragma unroll
    for (int v = 0; v < BS / 64; ++v) c += wave_cnt[v][threadIdx.x];
    wg_count[(u64)blockIdx.x * RESHARD_MAX_WORLD + threadIdx.x] = c;
  }
}

// One workgroup.  wg_off[b][o] = run[o] + the states of owner o in the workgroups before b; then
// run[o] += the block's states of owner o.  A block is at most 2^20 states, so its counts fit 32 bits.
__global__ void __launch_bounds__(BS) orig_reshard_scan(const u32* wg_count, u32 nwg, u64* run, u64* wg_off) {
  __shared__ u32 wave_tot[BS / 64];
  const u32 per = (nwg + BS - 1) / BS, b0 = threadIdx.x * per;
  for (u32 o = 0; o < (u32)RESHARD_MAX_WORLD; ++o) {
    u32 mine = 0;
    for (u32 b = b0; b < b0 + per && b < nwg; ++b) mine += wg_count[(u64)b * RESHARD_MAX_WORLD + o];
    u32 total = 0;
    const u32 excl = block_excl_scan(mine, wave_tot, &total);
    const u64 base = run[o];
    u64 at = base + excl;
    for (u32 b = b0; b < b0 + per && b < nwg; ++b) {
      wg_off[(u64)b * RESHARD_MAX_WORLD + o] = at;
      at += wg_count[(u64)b * RESHARD_MAX_WORLD + o];
    }
    __syncthreads();   // every thread has read run[o]
    if (threadIdx.x == 0) run[o] = base + total;
  }
}

struct ReshardPlaceArgs {
  const u32* in_states;          // the block: [n][NWP]
  const u64* in_meta;            // [n] parent pointers with source ids
  const unsigned char* owner;    // [n] (orig_reshard_classify)
  const u64* wg_off;             // [workgroups][8] (orig_reshard_scan)
  u64 n, pos0;                   // states in the block, canonical position of its first one in the level
  u64 level_size, prev_size;     // the level's and the previous level's states (the maps' lengths)
  u64 owner_begin[RESHARD_MAX_WORLD];   // the states every owner received from the levels before
  ReshardLevel prev;             // the source's layout of the level before (world 0: none)
  const u64* map_prev;           // [prev_size] new ids of the level before, by canonical position
  u64* map_cur;                  // [level_size]
  u32 me;                        // the target rank whose store this is
  u32* states;                   // its store
  u64* meta;
  u64 cap;
  unsigned long long* ctr;
};

template <int NWP>
__global__ void __launch_bounds__(BS) orig_reshard_place(ReshardPlaceArgs a) {
  __shared__ u32 wave_cnt[BS / 64][RESHARD_MAX_WORLD];
  const u64 i = (u64)blockIdx.x * BS + threadIdx.x;
  const int lane = __lane_id(), wave = threadIdx.x >> 6;
  const bool valid = i < a.n;
  const u32 own = valid ? (u32)a.owner[i] : ~0u;
  u32 in_wave = 0;
  u64 begin = 0;
#pragma unroll
  for (u32 o = 0; o < (u32)RESHARD_MAX_WORLD; ++o) {
    const unsigned long long b = __ballot(own == o);
    if (own == o) { in_wave = (u32)__popcll(b & ((1ull << lane) - 1)); begin = a.owner_begin[o]; }
    if (lane == 0) wave_cnt[wave][o] = (u32)__popcll(b);
  }
  __syncthreads();
  if (!valid || own >= (u32)RESHARD_MAX_WORLD) return;
  u32 before = 0;
  for (int v = 0; v < wave; ++v) before += wave_cnt[v][own];
  const u64 idx = a.wg_off[(u64)blockIdx.x * RESHARD_MAX_WORLD + own] + before + in_wave;
  const u64 pos = a.pos0 + i;
  if (pos < a.level_size) a.map_cur[pos] = reshard_new_id(own, begin, idx);
  // every rank checks every parent pointer (all ranks refuse a bad file alike); the owner stores
  u64 m = a.in_meta[i];
  if (m != ~0ull) {
    u64 ppos = 0;
    if (reshard_position(a.prev, m >> META_GID_SHIFT, ppos) && ppos < a.prev_size) m = reshard_meta(m, a.map_prev[ppos]);
    else { atomicOr(&a.ctr[K_ERR], (unsigned long long)OE_RESHARD_PARENT); return; }
  }
  if (own != a.me) return;
  const u64 dst = begin + idx;
  if (dst >= a.cap) { atomicOr(&a.ctr[K_ERR], (unsigned long long)OE_CAP_STORE); return; }
  const uint4* src = reinterpret_cast<const uint4*>(a.in_states + i * NWP);
  uint4* o4 = reinterpret_cast<uint4*>(a.states + dst * NWP);
#pragma unroll
  for (int q = 0; q < NWP / 4; ++q) o4[q] = src[q];
  a.meta[dst] = m;
}
