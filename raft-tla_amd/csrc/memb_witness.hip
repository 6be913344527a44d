// raftmc — continue mode for tlc_membership/raft.tla: the first counterexample of every listed
// invariant from one BFS (raftmc's own semantics, not TLC's -continue).  Included by
// memb_backend.hip (its BS, EV_* kinds, MGenArgs and CellRegions).
//
// In continue mode the BFS kernels run with no invariant (MembRuntime::n_inv = 0), so the search is the
// one of a cfg without INVARIANTS, and the two kernels here evaluate the invariants that are still
// pending -- a 32-bit mask of cfg positions, a kernel argument and so wave-uniform -- one by one
// (S::inv per position, never check_invariants' first hit) on the successors TLC checks:
//
//   memb_witness_new   lane per new state of the chunk, after memb_materialize: the stored state
//                      without its bag (no invariant reads the bag) and its (parent, slot) from meta
//   memb_witness_oom   lane per out-of-model successor (MC_COMPAT_INV_OUT_OF_MODEL): the cells_oom
//                      lists memb_expand wrote, re-derived as memb_oom_check does
//
// Both reduce the same way: wit[q] is the minimum key of a successor violating position q, wit[32]
// the minimum event word (key << 2 | EV_INV_ERROR) of one on which an invariant failed to evaluate.
// A scenario flag stays set in every descendant, so in the chunk where it first shows thousands of
// lanes hit the same position: the minimum is taken in LDS per workgroup (a read filters the lanes
// that cannot lower it, atomicMin the rest) and one global atomicMin per touched position and
// workgroup follows.  A position that has its witness leaves the mask from the next chunk on.
// (no includes and no namespace of its own: the text sits inside memb_backend.hip's namespace rmc)

enum { WIT_FATAL = 32, WIT_N = 33 };

struct MWitArgs {
  const u32* states;           // the store, indexed by global id
  const u64* meta;             // memb_witness_new: parent << 20 | action << 10 | slot of the new states
  u64 first, n_new;            // memb_witness_new: the chunk's new states [first, first + n_new)
  u64 level_begin;             // store index of rank 0 of the level
  MembRuntime rt;              // the cfg's invariants (inv_order, n_inv), unlike the BFS kernels' copy
  u32 pending;                 // cfg positions still without a witness
  unsigned long long* wit;     // [WIT_N], ~0 before the chunk
};

__device__ __forceinline__ void witness_init(unsigned long long* wmin) {
  for (int t = threadIdx.x; t < WIT_N; t += BS) wmin[t] = ~0ull;
  __syncthreads();
}

// the pending invariants on one checked successor (key: its position in TLC's enumeration order)
template <class S>
__device__ __forceinline__ void witness_eval(const typename S::Work& t, const MembRuntime& rt, u32 pending, u64 key,
                                             unsigned long long* wmin) {
  for (u32 m = pending; m; m &= m - 1) {   // (wave-uniform)
    const u32 q = (u32)__builtin_ctz(m);
    const u64 w = q < 8 ? rt.inv_order[0] : q < 16 ? rt.inv_order[1] : q < 24 ? rt.inv_order[2] : rt.inv_order[3];
    const int id = (int)((w >> (8 * (q & 7))) & 255u);
    const int r = S::inv(t, id, rt);
    if (r == IV_OK) continue;
    unsigned long long* const dst = &wmin[r == IV_BAD ? q : (u32)WIT_FATAL];
    if (key < __hip_atomic_load(dst, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) atomicMin(dst, (unsigned long long)key);
  }
}

__device__ __forceinline__ void witness_flush(const unsigned long long* wmin, unsigned long long* wit) {
  __syncthreads();
  for (int t = threadIdx.x; t < WIT_N; t += BS) {
    const unsigned long long k = wmin[t];
    if (k != ~0ull) atomicMin(&wit[t], t == WIT_FATAL ? ((k << 2) | EV_INV_ERROR) : k);
  }
}

template <class S>
__global__ void __launch_bounds__(BS) memb_witness_new(MWitArgs a) {
  using W = typename S::Work;
  __shared__ unsigned long long wmin[WIT_N];
  witness_init(wmin);
  const u64 i = (u64)blockIdx.x * BS + threadIdx.x;
  if (i < a.n_new) {
    const u64 g = a.first + i, meta = a.meta[g];
    const u64 key = ((meta >> 20) - a.level_begin) * (u64)S::NSLOT + (meta & 1023);
    const uint2* src = reinterpret_cast<const uint2*>(a.states + g * S::NWP);
    u32 w[S::BAGW];
#pragma unroll
    for (int q = 0; q < S::BAGW / 2; ++q) { const uint2 v = src[q]; w[2 * q] = v.x; w[2 * q + 1] = v.y; }
    W t;
    S::unpack_nobag(w, t);
    witness_eval<S>(t, a.rt, a.pending, key, wmin);
  }
  witness_flush(wmin, a.wit);
}

// (a: memb_expand's arguments of the chunk; its rt is the BFS kernels' copy, w.rt lists the invariants)
template <class S>
#ifndef RMC_MWIT_WAVES
#define RMC_MWIT_WAVES 4   // memb_oom_check's occupancy target (DESIGN.md §10 has the compiler's report)
#endif
__global__ void __launch_bounds__(BS) __attribute__((amdgpu_waves_per_eu(RMC_MWIT_WAVES))) memb_witness_oom(MGenArgs a, MWitArgs w) {
  using W = typename S::Work;
  constexpr int NWP = S::NWP;
  __shared__ unsigned long long wmin[WIT_N];
  witness_init(wmin);
  const CellRegions cr(a.cell_count + 8 * blockIdx.x + 4, 64 * S::NSLOT);
  const u32 n = cr.n;
  const u32* cells = a.cells_oom + (u64)blockIdx.x * (BS * S::NSLOT);
  for (u32 i = threadIdx.x; i < n; i += BS) {
    const u32 cell = cells[cr.at(i)];
    const u64 slot = cell / a.chunk_count, st = cell - slot * a.chunk_count;
    int k, sub;
    S::inst_of_slot((int)slot, k, sub);
    const uint2* src = reinterpret_cast<const uint2*>(a.states + (a.chunk_begin + st) * NWP);
    u32 pw[S::BAGW];
#pragma unroll
    for (int q = 0; q < S::BAGW / 2; ++q) { const uint2 v = src[q]; pw[2 * q] = v.x; pw[2 * q + 1] = v.y; }
    const int bi = S::bag_slot_of(k);
    u64 xent = S::EMPTY;
    if (bi >= 0) { const uint2 v = src[S::BAGW / 2 + bi]; const u64 x = (u64)v.x | (u64)v.y << 32; xent = x ? x : S::EMPTY; }
    W s, t;
    S::unpack_nobag(pw, s);
    u32 err = 0;
    typename S::Delta d;
    S::template apply_nobag<false>(s, k, sub, xent, t, d, err, a.rt);
    witness_eval<S>(t, w.rt, w.pending, (a.rank0 + st) * (u64)S::NSLOT + slot, wmin);
  }
  witness_flush(wmin, w.wit);
}
