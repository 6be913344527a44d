// raftmc — simulation mode (TLC -simulate) for thirdparty/raft_original.tla: seeded random walks
// of bounded depth on gfx950.  Included by orig_backend.hip (its BS, EV_* kinds and HIPCHK).
//
// A walk needs no seen-set, no store and no dedup: each lane carries one state (S::Work) from Init
// through at most depth - 1 steps in registers; the only global traffic is a handful of counters
// and one event word per workgroup, at the end.  Semantics: at every step all NI
// action instances are evaluated in apply's order (allLogs' applied as orig_generate applies it);
// every enabled instance is one generated state (per-action counts; equal successors are not merged,
// as in TLC's simulator); invariants are checked on every generated successor (in-model ones only
// when MC_COMPAT_INV_OUT_OF_MODEL is cleared); the walk moves to one successor chosen uniformly
// among the in-model ones (sim_rng.h: counter-based draws, reservoir rule) and ends at `depth`
// states or when no successor is in the model.  A walk whose step raises an event (violation,
// evaluation error, deadlock) ends there; the batch's event is the minimum (trace length, walk,
// instance) through one 64-bit atomicMin, and the host replays that walk from (seed, walk) with the
// same spec code (sim_replay) for the counterexample: no path is stored on the device.
//
// orig_simulate<S>: one lane per walk, all steps in one launch.  The instance loop is wave-uniform
// (k is a scalar, so apply's dispatch and the bag slot selects are scalar work, as in orig_generate's
// second section); a RequestVote instance no lane of the wave can take (S::request_vote_mask) and the
// leader range [LEAD_LO, LEAD_HI) of a wave without leader work (S::leader_work) are skipped by a
// wave ballot; DuplicateMessage / DropMessage successors that BoundedMessages puts out of the model
// are counted without being built (S::quick_out_of_model: no invariant reads the bag, S::inv_frame).
// The walk's current state satisfies every invariant (a violating successor ends the walk), so a
// successor is checked against the invariants its action can change only (S::inv_frame).
//
// Picking the successor: the reservoir keeps the instance index (one register), and after the
// instance loop each lane applies its own instance once more, S::apply with a per-lane k (RMC_SIM_SELECT
// 2).  A per-lane instance turns apply's dispatch into vector work (orig_generate's header: 19.5 vs
// 14.5 ms when every instance went that way), but here it is one call per step against NI uniform
// ones, and only two Works are live.  Measured on MI355X, c2.cfg, 2^20 walks of depth 64 (66.1M
// steps, 1,313M successors; median of 30 runs, the builds alternating; profiles/sim_select_ab.json)
// and the compiler's resource report (profiles/sim_resources.json; VGPRs / spilled VGPRs / waves per
// SIMD for C2 (3,2,3,2,5), then for (5,2,2,4,6)):
//   2  index + one per-lane apply (this one)    13.61 ms    94 / 0 / 5    147 / 0 / 3
//   0  reservoir-keep the successor Work itself 14.20 ms   128 / 16 / 4   238 / 0 / 2
//      (one pass, but a third Work live and a conditional copy of it per in-model successor: it
//      misses orig_generate's occupancy target for NW <= 15 -- 128 VGPRs only by spilling 16)
//   1  index + a second wave-uniform pass in which each lane applies only its own instance (a trip
//      per distinct index in the wave)           16.69 ms   111 / 0 / 4   150 / 0 / 3
// Not built: count, draw once, re-run to the r-th in-model instance -- the second pass of 1, except
// that it cannot skip: every lane re-evaluates apply and in_model for each instance up to its r-th,
// so it costs strictly more than 1 at the same register count.
// (no includes and no namespace of its own: the text sits inside orig_backend.hip's namespace rmc)
#ifndef RMC_SIM_SELECT
#define RMC_SIM_SELECT 2
#endif

enum { SK_EVENT = 0, SK_ERR = 1, SK_STEPS = 2, SK_MAXLEN = 3, SK_ACT = 4, SK_NCTR = SK_ACT + OA_NACT };

struct SimArgs {
  u64 walk0, nwalks;           // the batch: walks walk0 .. walk0 + nwalks - 1
  u64 seed;
  u32 depth;                   // states per walk at most, Init included (>= 1)
  OrigRuntime rt;
  u32 inv_oom, deadlock;
  unsigned long long* ctr;     // [SK_NCTR]; SK_EVENT starts at ~0, the others at 0
};

template <class S>
__global__ void __launch_bounds__(BS) __attribute__((amdgpu_waves_per_eu(S::NW <= 15 ? 4 : 1))) orig_simulate(SimArgs a) {
  using W = typename S::Work;
  static_assert(S::NI <= 255, "the event word holds the instance in 8 bits");
  __shared__ unsigned int lds_cnt[OA_NACT + 2];   // per-action generated, steps, longest walk
  for (int t = threadIdx.x; t < OA_NACT + 2; t += BS) lds_cnt[t] = 0;
  __syncthreads();
  const u64 tid = (u64)blockIdx.x * BS + threadIdx.x;
  const u64 walk = a.walk0 + tid;
  bool alive = tid < a.nwalks;
  W s;
  S::init(s);
  u32 len = alive ? 1u : 0u, nsteps = 0, err = 0;
  unsigned long long ev = ~0ull;
#pragma unroll 1
  for (u32 step = 0; step + 1 < a.depth; ++step) {
    if (!__ballot(alive)) break;
    u64 al[S::AW];
    S::all_logs_next(s, al);
    const u64 key = sim_step_key(a.seed, walk, step);
    const u32 rvm = alive ? S::request_vote_mask(s) : 0u;
    const bool lead = __ballot(alive && S::leader_work(s)) != 0ull;   // wave-uniform
    u32 nsucc = 0, j = 0;
    int evk = -1;
#if RMC_SIM_SELECT == 0
    W kept = s;
#else
    int kept_k = -1;
#endif
    if (alive) ++nsteps;
#pragma unroll 1
    for (int kk = 0; kk < S::NI; ++kk) {
      if (kk == S::LEAD_LO && !lead) kk = S::LEAD_HI;   // no Leader, no Candidate with a quorum in this wave
      const int k = kk;                                // wave-uniform
      if (k >= 2 * S::N && k < 2 * S::N + S::N * S::N && !__ballot((rvm >> (k - 2 * S::N)) & 1u)) continue;
      if (!alive) continue;
      const int qa = S::quick_out_of_model(s, k, a.rt);
      if (qa >= 0) {      // generated, out of the model, no invariant to check: counted only
        ++nsucc;
        atomicAdd(&lds_cnt[qa], 1u);
        continue;
      }
      W t;
      const int act = S::apply(s, k, t, err);
      if (act < 0) continue;
#pragma unroll
      for (int q = 0; q < S::AW; ++q) t.allLogs[q] = al[q];
      ++nsucc;
      atomicAdd(&lds_cnt[act], 1u);
      const bool inm = S::in_model(t, a.rt);
      if ((inm || a.inv_oom) && evk < 0 &&
          (action_step_violated<S>(s, t, k, act, a.rt) || S::violated(t, a.rt.invariants & S::inv_frame(act))))
        evk = k;
      if (inm) {
        ++j;
#if RMC_SIM_SELECT == 0
        if (sim_take(key, j)) kept = t;
#else
        if (sim_take(key, j)) kept_k = k;
#endif
      }
    }
    // how the step ends for this walk
    bool go = false;
    if (alive) {
      if (err & OE_EVAL_LOG_INDEX) {
        const u64 e = sim_event(len, walk, 0u, EV_NEXT_ERROR);
        ev = e < ev ? e : ev;
      } else if (err) {
        // compiled-capacity limit: reported through SK_ERR below
      } else if (evk >= 0) {
        ++len;
        const u64 e = sim_event(len, walk, (u32)evk, EV_VIOLATION);
        ev = e < ev ? e : ev;
      } else if (nsucc == 0) {
        if (a.deadlock) { const u64 e = sim_event(len, walk, 0u, EV_DEADLOCK); ev = e < ev ? e : ev; }
      } else if (j != 0) {
        go = true;
      }
      alive = go;
    }
#if RMC_SIM_SELECT == 0
    if (go) { s = kept; ++len; }
#elif RMC_SIM_SELECT == 2
    if (go) {   // one apply with a per-lane instance
      W t;
      u32 e2 = 0;
      (void)S::apply(s, kept_k, t, e2);
#pragma unroll
      for (int q = 0; q < S::AW; ++q) t.allLogs[q] = al[q];
      s = t;
      ++len;
    }
#else
#pragma unroll 1
    for (int k = 0; k < S::NI; ++k) {
      const bool mine = go && kept_k == k;
      if (!__ballot(mine)) continue;
      if (mine) {
        W t;
        u32 e2 = 0;
        (void)S::apply(s, k, t, e2);
#pragma unroll
        for (int q = 0; q < S::AW; ++q) t.allLogs[q] = al[q];
        s = t;
        ++len;
      }
    }
#endif
  }
  const u32 cap_err = err & ~(u32)OE_EVAL_LOG_INDEX;
  if (cap_err) atomicOr(&a.ctr[SK_ERR], (unsigned long long)cap_err);
  if (ev != ~0ull) atomicMin(&a.ctr[SK_EVENT], ev);
  if (nsteps) atomicAdd(&lds_cnt[OA_NACT], nsteps);
  if (len) atomicMax(&lds_cnt[OA_NACT + 1], len);
  __syncthreads();
  for (int t = threadIdx.x; t < OA_NACT; t += BS)
    if (lds_cnt[t]) atomicAdd(&a.ctr[SK_ACT + t], (unsigned long long)lds_cnt[t]);
  if (threadIdx.x == 0) {
    if (lds_cnt[OA_NACT]) atomicAdd(&a.ctr[SK_STEPS], (unsigned long long)lds_cnt[OA_NACT]);
    if (lds_cnt[OA_NACT + 1]) atomicMax(&a.ctr[SK_MAXLEN], (unsigned long long)lds_cnt[OA_NACT + 1]);
  }
}

// One walk replayed on the host from (seed, walk) with the spec code the kernel runs: its states
// (the violating successor last, when the walk ends in a violation), the action of every step and
// the walk's event word (~0: none).  The counterexample of a run and mc_sim_walk come from here.
template <class S>
struct SimWalk {
  std::vector<typename S::Work> states;
  std::vector<int> acts;   // acts[k]: the action that led to states[k + 1]
  u64 event = ~0ull;
  u32 err = 0;             // OE_* flags of the step that ended the walk
};

template <class S>
void sim_replay(const OrigRuntime& rt, bool inv_oom, bool deadlock, u64 seed, u64 walk, u32 depth, SimWalk<S>& out) {
  using W = typename S::Work;
  W s;
  S::init(s);
  out = SimWalk<S>();
  out.states.push_back(s);
  for (u32 step = 0; step + 1 < depth; ++step) {
    u64 al[S::AW];
    S::all_logs_next(s, al);
    const u64 key = sim_step_key(seed, walk, step);
    u32 nsucc = 0, j = 0, err = 0;
    int evk = -1, ev_act = -1, kept_act = -1;
    W kept = s, bad = s;
    for (int k = 0; k < S::NI; ++k) {
      W t;
      const int act = S::apply(s, k, t, err);
      if (act < 0) continue;
      for (int q = 0; q < S::AW; ++q) t.allLogs[q] = al[q];
      ++nsucc;
      const bool inm = S::in_model(t, rt);
      bool viol = S::violated(t, rt.invariants) != 0u;
      if constexpr (S::ACTIONS) viol = viol || S::violated_action(s, t, k, rt.action_props) != 0u;   // every listed property, unframed
      if ((inm || inv_oom) && evk < 0 && viol) { evk = k; ev_act = act; bad = t; }
      if (inm && sim_take(key, ++j)) { kept = t; kept_act = act; }
    }
    const u64 len = out.states.size();
    if (err) {
      out.err = err;
      if (err & OE_EVAL_LOG_INDEX) out.event = sim_event(len, walk, 0u, EV_NEXT_ERROR);
      return;
    }
    if (evk >= 0) {
      out.states.push_back(bad); out.acts.push_back(ev_act);
      out.event = sim_event(len + 1, walk, (u32)evk, EV_VIOLATION);
      return;
    }
    if (nsucc == 0) { if (deadlock) out.event = sim_event(len, walk, 0u, EV_DEADLOCK); return; }
    if (j == 0) return;
    s = kept;
    out.states.push_back(s); out.acts.push_back(kept_act);
  }
}
