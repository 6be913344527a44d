// raftmc — SYMMETRY Permutations(Server) for raft_original: included by orig_backend.hip (inside
// namespace rmc, after the kernels it shares GenArgs, ev_word, probe_batch and the K_* counters
// with).  DESIGN.md §11.
//
// Under SYMMETRY the seen-set holds one fingerprint per orbit (S::fp_sym, orig_spec.h) and nothing
// else changes: the state kept, stored, expanded and printed is the successor as generated (what
// TLC does), so the records of this kernel are the records of orig_generate -- (fp, lane << 8 |
// instance) in the wave's own region -- and dedup, the LDS filter, winner selection, materialize
// (which re-derives a winner from (parent, instance)) and the stop-point kernels run unchanged.

// One lane per frontier state, a wave-uniform loop over ALL the action instances (the leader range
// included: no orig_generate_lead pass, K_LEAD stays 0).  Successor, constraints, TLC generated
// counts and out-of-model invariants as in orig_generate; the fingerprint of an in-model successor
// is S::fp_sym of the successor itself.  No incremental hash and no "successor equals its parent"
// skip: the orbit fingerprint is not a sum over packed words, and a successor in its parent's
// orbit is found in the seen-set like any other duplicate.
template <class S>
__global__ void __launch_bounds__(BS) orig_generate_sym(GenArgs a) {
  using W = typename S::Work;
  constexpr int NWP = (S::NW + 3) & ~3;
  __shared__ unsigned int lds_cnt[OA_NACT + 1];   // per-action generated, in-model total
  for (int t = threadIdx.x; t < OA_NACT + 1; t += BS) lds_cnt[t] = 0;
  __syncthreads();
  const u64 tid = (u64)blockIdx.x * BS + threadIdx.x;
  const bool active = tid < a.chunk_count;
  const u64 gid = a.gid0 + tid;
  const int lane = __lane_id();
  const u32 wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const u64 wreg = (u64)blockIdx.x * (BS * S::NI) + (u64)wave * (64 * S::NI);   // a lane leaves <= NI records
  u64* rfp = a.rfp + wreg;
  unsigned short* rkey = a.rkey + wreg;
  u32 wcount = 0;
  W s;
  u64 al[S::AW];
  u32 err = 0, nsucc = 0, nin = 0;
  unsigned long long ev = ~0ull;
  if (active) {
    u32 w[NWP];
    const uint4* src = reinterpret_cast<const uint4*>(a.states + (a.chunk_begin + tid) * NWP);
#pragma unroll
    for (int q = 0; q < NWP / 4; ++q) { const uint4 v = src[q]; w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w; }
    S::unpack(w, s);
    S::all_logs_next(s, al);
  } else {
    S::init(s);
#pragma unroll
    for (int q = 0; q < S::AW; ++q) al[q] = 0;
  }
#pragma unroll 1
  for (int k = 0; k < S::NI; ++k) {   // k is wave-uniform
    u64 fp = 0;
    bool have = false;
    const int qa = active ? S::quick_out_of_model(s, k, a.rt) : -1;
    if (qa >= 0) {      // generated, out of the model, no invariant to check: counted only
      ++nsucc;
      atomicAdd(&lds_cnt[qa], 1u);
    } else if (active) {
      W t;
      const int act = S::apply(s, k, t, err);
      if (act >= 0) {
#pragma unroll
        for (int q = 0; q < S::AW; ++q) t.allLogs[q] = al[q];
        ++nsucc;
        atomicAdd(&lds_cnt[act], 1u);
        const bool step_bad = action_step_violated<S>(s, t, k, act, a.rt);
        if (S::in_model(t, a.rt)) {
          ++nin;
          fp = S::fp_sym(t, a.seed);
          have = true;
          if (step_bad) { const u64 e = ev_word(gid, (u32)k, EV_VIOLATION); ev = e < ev ? e : ev; }
        } else if (a.inv_oom && (step_bad || S::violated(t, a.rt.invariants & S::inv_frame(act)))) {
          const u64 e = ev_word(gid, (u32)k, EV_VIOLATION);
          ev = e < ev ? e : ev;
        }
      }
    }
    // this wave's in-model successors of the trip into its record region (one ballot, consecutive stores)
    const u64 mask = __ballot(have);
    if (have) {
      const u32 idx = wcount + __builtin_amdgcn_mbcnt_hi((u32)(mask >> 32), __builtin_amdgcn_mbcnt_lo((u32)mask, 0u));
      rfp[idx] = fp;
      rkey[idx] = (unsigned short)((threadIdx.x << 8) | (unsigned)k);
    }
    wcount += (u32)__popcll(mask);
  }
  if (active) {
    if (err & OE_EVAL_LOG_INDEX) { const u64 e = ev_word(gid, 0, EV_NEXT_ERROR); ev = e < ev ? e : ev; }
    if (nsucc == 0 && a.deadlock) { const u64 e = ev_word(gid, 0, EV_DEADLOCK); ev = e < ev ? e : ev; }
  }
  const u32 cap_err = err & ~(u32)OE_EVAL_LOG_INDEX;   // compiled-capacity limits, not TLC semantics
  if (cap_err) {
    atomicOr(&a.ctr[K_ERR], (unsigned long long)cap_err);
    atomicCAS(&a.ctr[K_ERRGID], 0ull, (unsigned long long)(gid + 1));
  }
  if (ev != ~0ull) atomicMin(&a.ctr[K_EVENT], ev);
  if (nin) atomicAdd(&lds_cnt[OA_NACT], nin);
  __syncthreads();
  for (int t = threadIdx.x; t < OA_NACT; t += BS)
    if (lds_cnt[t]) atomicAdd(&a.ctr[K_ACT + t], (unsigned long long)lds_cnt[t]);
  if (threadIdx.x == 0 && lds_cnt[OA_NACT]) atomicAdd(&a.ctr[K_GEN_IN], (unsigned long long)lds_cnt[OA_NACT]);
  if (lane == 0) a.rcnt[blockIdx.x * 4 + wave] = wcount;
}

// orig_reinsert under SYMMETRY (-recover): the orbit fingerprint of every stored state back into
// the zeroed seen-set
template <class S, int STRIDE>
__global__ void __launch_bounds__(BS) orig_reinsert_sym(const u32* states, u64 n, u64* table, u64 mask, u64 seed,
                                                        unsigned long long* ctr) {
  constexpr int NWP = (S::NW + 3) & ~3;
  const u64 i = (u64)blockIdx.x * BS + threadIdx.x;
  if (i >= n) return;
  u32 w[NWP];
#pragma unroll
  for (int q = 0; q < NWP; ++q) w[q] = states[i * NWP + q];
  typename S::Work s;
  S::unpack(w, s);
  const u64 fp[1] = {S::fp_sym(s, seed)}, nk[1] = {~0ull};
  u64 pos[1];
  u32 err = 0;
  probe_batch<1, STRIDE == 2, STRIDE>(table, mask, fp, nk, pos, err);
  if (err) atomicOr(&ctr[K_ERR], (unsigned long long)err);
}
