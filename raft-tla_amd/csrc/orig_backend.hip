// raftmc — gfx950 BFS backend for thirdparty/raft_original.tla.
//
// TLC's single-worker FIFO order, reproduced on a data-parallel GPU.  Every successor has the
// key  (global id of its parent) << 8 | instance,  where the instance index is its position in
// TLC's enumeration of the Next disjuncts (raft_original.tla:453-462; the order-preserving
// message codes of orig_spec.h make bag slot order the order of `\E m \in DOMAIN messages`).
// States are stored level by level in key order, so parent ids increase in FIFO order and the
// key is globally monotone over the whole search: the seen-set keeps the MINIMUM key per
// fingerprint (16-B entries {fp, ~key}, atomicMax on the complement), i.e. TLC's first-found
// parent, and every count, parent pointer, counterexample and stop point is TLC's.
//
// One BFS level is processed in frontier chunks.  A chunk's kernels run in this order; on the
// sharded, native and FIFO paths and on small levels all on one stream, on the large levels of the
// single-GPU -workers N search with step 1 of the next sub-chunk on a second stream beside steps 2-6
// of this one (run(), "Generate beside dedup"):
//
//  1. orig_generate  (compute): one lane per frontier state, a wave-uniform loop over the
//     action instances; constraint filter, TLC generated counts, out-of-model invariants (TLC
//     semantics, [ext] switch), canonical pack and FP64 of each in-model successor.  The
//     workgroup's in-model successors are compacted (wave ballot + one LDS atomic per wave and
//     instance) into its own record region: fp (8 B) + local key lane << 8 | instance (2 B).
//  2. orig_dedup     (HBM random access): workgroup b takes generate-workgroup b's records; a
//     workgroup-local LDS set {fp, min local key} merges the successors its 256 parents produce
//     more than once (diamonds of commuting actions, ~half of C2's), then every distinct fp of
//     the set probes the seen-set, 16 in flight per thread (lock-free linear probing over 16-B
//     entries, CAS insert of the fp, atomicMax of ~key).  Inserted entries' positions are
//     appended (one global atomic per workgroup).
//  3. orig_mark      lane per inserted entry: its final key names TLC's first-found producer;
//     set that (parent, instance) bit of the winner mask, count per workgroup of parents.
//  4. orig_scan      exclusive scan of the per-workgroup winner counts (one workgroup).
//  5. orig_materialize workgroup per 256 parents: winners in key order (parent-major, instance
//     order), re-derived from (parent, instance), stored with their parent pointers at their
//     FIFO position; invariants of the new states.
//  6. orig_advance   the level's running count of new states (between the chunks of a level; the
//     host adds the last chunk's count itself).
//
// The first *event* of a level in key order — a TLC evaluation error while computing a
// parent's successors, a deadlock, an invariant violation (new or out-of-model successor) — is
// a 64-bit atomicMin of key << 2 | kind; the host re-derives that successor with the same
// spec code and reproduces TLC's stop point (generated / distinct / per-action counts /
// left-on-queue) and counterexample.  All distinct states stay resident in HBM (completed
// levels spill to host memory when the store fills); traces chase parent pointers.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <sstream>
#include <type_traits>

#include "../../include/raftmc.h"
#include "backend.h"
#include "chunk_plan.h"
#include "fp_gap.h"
#include "orig_spec.h"
#include "orig_text.h"
#include "rccl_api.h"
#include "reshard_plan.h"
#include "shard_transport.h"
#include "sim_rng.h"
#include "state_store.h"

namespace rmc {

enum {
  K_NEW = 0, K_GEN_IN = 1, K_ERR = 2, K_EVENT = 3, K_ERRGID = 4, K_INS = 5, K_CHUNK_NEW = 6, K_LEVEL_NEW = 7,
  K_ACT = 8, K_PROF = K_ACT + 2 * OA_NACT,   // K_PROF: phase timers (RAFTMC_PROF, slots 0..5)
  K_PROBES = K_PROF + 6,                       // seen-set probes issued (fingerprints that reached the table)
  K_LEAD = K_PROF + 7,                         // the chunk's leader-work parents (orig_generate_lead)
  K_NCTR = K_PROF + 8
};
enum { EV_NEXT_ERROR = 0, EV_DEADLOCK = 1, EV_INV_ERROR = 2, EV_VIOLATION = 3 };
enum { OE_CAP_STORE = 0x100, OE_TABLE_FULL = 0x200 };
// Seen-set batches and the LDS filter (round 5, profiles/r05_dedup_ab.txt r5x-r6a): 4 probes in flight
// per thread at 50 VGPRs and a 2048-slot filter (18.4 KB of LDS) give 8 workgroups per CU, the wave
// limit, where 8 probes at 92 VGPRs and 4096 slots (34.8 KB) gave 4: orig_dedup_plain 11.5 -> 10.4 ms
// per C2 run although 3.5% more fingerprints get past the smaller filter (351M probes, not 339M); the
// FIFO path 35.9 -> 34.8 ms.  16 per thread (183 VGPRs) 16.4 ms, 1024 slots 11.1 ms.
constexpr int DEDUP_PER = 4;                  // probes in flight per dedup thread
constexpr int BS = 256;                       // workgroup size of every kernel (4 waves)
constexpr int LDS_FP_SLOTS = 2048;            // workgroup-local fingerprint set (8 B fp + 4 B key per slot)
// orig_dedup_plain beside a generate (profiles/r09_overlap_third_wave_ab.txt): 2 probes in
// flight per thread bring a wave from 56 to 32 VGPRs, so that 4 dedup waves and 3 generate waves (128 each)
// fill a SIMD's 512 where two generate waves fitted before, and the 4096-slot filter's 32 KB are what holds
// a CU to 4 dedup workgroups (of 160 KB): C2 22.3 -> 21.0 ms per run.  The filter is the launch's dynamic
// LDS: as a static array it tells the compiler that 4 waves per SIMD is the most, and the compiler then
// raises the wave's register allocation to the most that allows 4 (104, with 30 in use), which leaves no
// room for any generate wave (22.8 ms).
constexpr int OVERLAP_DEDUP_PER = 2;
constexpr int OVERLAP_LDS_FP_SLOTS = 4096;
constexpr unsigned OVERLAP_FILTER_LDS = OVERLAP_LDS_FP_SLOTS * 8;   // dynamic LDS of the launch beside a generate
constexpr int MAT_CAP = 2048;      // winners staged in LDS per materialize round
#ifndef RMC_RV_PATCH
#define RMC_RV_PATCH 0
#endif
#ifndef RMC_RV_WCOUNT
#define RMC_RV_WCOUNT 0
#endif
constexpr int SCAN_BS = 1024;      // orig_scan workgroup

// f(std::integral_constant<int, Q>) for Q = B .. E-1: a loop whose index is a compile-time constant
template <int B, int E, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (B < E) {
    f(std::integral_constant<int, B>{});
    static_for<B + 1, E>(f);
  }
}

// 64-bit event word: key << 2 | kind, key = parent gid << 8 | instance (gid < 2^40)
RMC_HD u64 ev_word(u64 gid, u32 inst, u32 kind) { return (((gid << 8) | (u64)inst) << 2) | (u64)kind; }

// Does the step (s, t) of instance k (action act) break a listed action property ([][A]_vars, orig_spec.h
// §14)?  Compiled into the kernels over WithActions<..> only (S::ACTIONS): in every other instantiation it
// is the constant false and leaves no code.  Only the properties the action can break are evaluated
// (S::act_frame).  A violation raises the event word of an invariant violation at the same key.
template <class S>
__device__ __forceinline__ bool action_step_violated(const typename S::Work& s, const typename S::Work& t, int k, int act,
                                                     const OrigRuntime& rt) {
  if constexpr (S::ACTIONS) {
    const u32 m = rt.action_props & S::act_frame(act);
    return m != 0u && S::violated_action(s, t, k, m) != 0u;
  } else {
    return false;
  }
}

struct GenArgs {
  const u32* states;           // device store [cap][NWP]
  u64 chunk_begin, chunk_count;   // device index of the chunk's first parent, parents
  u64 gid0;                    // global id of the chunk's first parent
  u64* rfp;                    // [nblk][BS * NI] fingerprints of in-model successors (per-workgroup region)
  unsigned short* rkey;        // [nblk][BS * NI] local key: lane << 8 | instance
  u32* rcnt;                   // [nblk][4] records per wave (wave w's region starts at w * 64 * NI)
  u64 seed;
  OrigRuntime rt;
  u32 inv_oom, deadlock;
  unsigned long long* ctr;
  u32* lead;                   // [chunk] parents with leader work (chunk index | 1 << 31 if no other successor)
};

// One lane per frontier state; successor, constraints, TLC generated counts, out-of-model invariants,
// canonical pack and FP64 in one pass.  (A split expand + full-lane fingerprint pipeline measured
// 51.4 vs 49.4 ms/run on C2: apply, not the pack + hash, dominates this spec.)  Three sections:
//  * RequestVote(i, j): each lane's enabled instances one per trip (per-lane instance);
//  * a wave-uniform loop over the other instances (Restart, Timeout, Receive; the leader instances
//    [LEAD_LO, LEAD_HI) are orig_generate_lead's): k is a scalar, so the instance decode and the bag
//    slot selects are scalar work;
//  * DuplicateMessage / DropMessage unrolled per bag slot, without apply or pack.
// In-model successors leave as compacted records: per instance a wave ballot and consecutive stores
// into the wave's own region (only ~21% of C2's instance slots carry an in-model successor).
// Rejected designs (measured on MI355X: DESIGN.md §4; their code is in the repository's history):
// instances binned by family for every family (19.5 vs 14.5 ms, round 4: a per-lane instance turns
// apply's whole dispatch into vector work), patch packing from the parent's words (14.45 vs 13.37 ms,
// round 5), per-wave aggregated action counts (+1.3 ms, round 2), DuplicateMessage / DropMessage
// through apply (13.37 -> 14.71 ms).
// 4 waves per SIMD (<= 128 VGPRs, no spill): 11.7 vs 13.4 ms per C2 run at 3 (round 5); 5 spills.
// Larger states (C5: 24 words) get no hint and keep the plain hash (the base terms would cost them
// occupancy: 45 vs 38 ms of expand time for C5 to depth 12).
template <class S>
__global__ void __launch_bounds__(BS) __attribute__((amdgpu_waves_per_eu(S::GEN_WAVES))) orig_generate(GenArgs a) {
  using W = typename S::Work;
  constexpr int NW = S::NW, NWP = (S::NW + 3) & ~3;
  __shared__ unsigned int lds_cnt[OA_NACT + 1];   // per-action generated, in-model total
  for (int t = threadIdx.x; t < OA_NACT + 1; t += BS) lds_cnt[t] = 0;
  __syncthreads();
  const u64 tid = (u64)blockIdx.x * BS + threadIdx.x;
  const bool active = tid < a.chunk_count;
  const u64 gid = a.gid0 + tid;
  const int lane = __lane_id();
  // each wave appends to its own region: the running count is wave-uniform, no LDS atomic per instance
  const u32 wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform (SGPR) region base
  const u64 wreg = (u64)blockIdx.x * (BS * S::NI) + (u64)wave * (64 * S::NI);
  u64* rfp = a.rfp + wreg;
  unsigned short* rkey = a.rkey + wreg;
  u32 wcount = 0;
  W s;
  u64 al[S::AW];
  u32 err = 0, nsucc = 0, nin = 0;
  unsigned long long ev = ~0ull;
  // the parent's packed words with allLogs' (every successor carries allLogs \cup {log[i]},
  // raft_original.tla:464) and their fingerprint terms: successors re-hash changed words only
  constexpr bool INC = NW <= 16;
  u32 bw[INC ? NW : 1];
  FpBase<INC ? NW : 2> fb;
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
  // bw = the parent with allLogs' (what every successor carries); a successor whose words equal bw is
  // the parent itself only when allLogs' = allLogs (no log of the parent is new to allLogs)
  bool al_same = true;
#pragma unroll
  for (int q = 0; q < S::AW; ++q) al_same &= al[q] == s.allLogs[q];
  if constexpr (INC) {
    W b = s;
#pragma unroll
    for (int q = 0; q < S::AW; ++q) b.allLogs[q] = al[q];
    S::pack(b, bw);
    fb.init(bw, a.seed);
  }
  // an in-model successor t (allLogs' applied): its fingerprint, and whether it leaves a record -- a
  // successor equal to its parent (Restart(i) of a server already in the reset state, allLogs' =
  // allLogs) is in the seen-set under an older key: no record, no probe (C2: 351M -> 313M seen-set
  // probes per run, round 6)
  auto fingerprint = [&](const W& t, u64& fp) -> bool {
    u32 pw[NW];
    S::pack(t, pw);
    if constexpr (INC) {
      bool changed;
      fp = fb.fp(pw, bw, a.seed, changed);
      return changed || !al_same;
    } else {
      fp = fp64(pw, a.seed);
      return true;
    }
  };
  // this wave's in-model successors of one trip into its record region (one ballot, consecutive stores)
  auto append = [&](bool have, u64 fp, int k) {
    const u64 mask = __ballot(have);
    if (have) {
      const u32 idx = wcount + __builtin_amdgcn_mbcnt_hi((u32)(mask >> 32), __builtin_amdgcn_mbcnt_lo((u32)mask, 0u));
      rfp[idx] = fp;
      rkey[idx] = (unsigned short)((threadIdx.x << 8) | (unsigned)k);
    }
    wcount += (u32)__popcll(mask);
  };
  // leader work (S::leader_work: a Leader or a Candidate with a quorum, ~1% of C2's states) is
  // left to orig_generate_lead, which runs those instances on full waves of just such parents: here
  // a wave with one leader lane would pay all of [LEAD_LO, LEAD_HI) for it (measured: a third of
  // this kernel's time for 0.7% of C2's successors)
  const bool lead = active && S::leader_work(s);
  {
    // RequestVote(i, j) [2N, 2N + N*N) (raft_original.tla:189-198): each lane's enabled instances one
    // per trip (S::request_vote_mask), so the wave runs as often as its busiest lane has RequestVote
    // instances instead of N*N times (C2: 6.3 trips per wave against 9, tests/native/orig_host_bfs.cpp
    // WAVE=64 "rv_waves"; orig_generate 11.1 -> 9.8 ms per run, round 6).  The handler is one short
    // function of (i, j) (S::request_vote), so a per-lane instance costs a few VALU ops here.
    u32 rvm = active ? S::request_vote_mask(s) : 0u;
#pragma unroll 1
    while (__ballot(rvm != 0u)) {
      const bool on = rvm != 0u;
      const int q = on ? __builtin_ctz(rvm) : 0;
      if (on) rvm &= rvm - 1u;
      const int k = 2 * S::N + q;
      bool have = false;
      u64 fp = 0;
      if (on) {
        W t = s;
        const int act = S::request_vote(s, q / S::N, q % S::N, t, err);
        if (act >= 0) {
#pragma unroll
          for (int w2 = 0; w2 < S::AW; ++w2) t.allLogs[w2] = al[w2];
          ++nsucc;
          if (!RMC_RV_WCOUNT) atomicAdd(&lds_cnt[act], 1u);
          if (S::in_model(t, a.rt)) {
            ++nin;
#if RMC_RV_PATCH
            if constexpr (INC) {
              // RequestVote changes only the bag: the parent's words with the bag re-packed, and only the
              // 64-bit words from the bag's first one re-hashed (both compile-time ranges)
              u32 pw[NW];
              S::pack_patch(t, 1u << S::PG_BAG, bw, pw);
              bool changed;
              fp = fb.template fp_tail<S::BAG_OFF / 64>(pw, bw, a.seed, changed);
              have = changed || !al_same;
            } else {
              have = fingerprint(t, fp);
            }
#else
            have = fingerprint(t, fp);
#endif
          }
          // out of the model: RequestVote writes only the bag, which no invariant reads (S::inv_frame)
        }
      }
      if (RMC_RV_WCOUNT) {   // every lane of the trip generates one RequestVote: one LDS atomic per wave
        const u64 gm = __ballot(on);
        if (lane == __ffsll((unsigned long long)gm) - 1) atomicAdd(&lds_cnt[OA_RequestVote], (unsigned)__popcll(gm));
      }
      append(have, fp, k);
    }
  }
  // DuplicateMessage / DropMessage [I_DUP, NI) change one message count and nothing else: with the
  // incremental fingerprint they are the unrolled section after this loop (no apply, no pack)
  constexpr int KEND = INC ? S::I_DUP : S::NI;
#pragma unroll 1
  for (int kk = 0; kk < KEND; ++kk) {
    if (kk == 2 * S::N) kk = S::LEAD_HI;   // RequestVote: the section above; leader work: orig_generate_lead
    const int k = kk;                      // wave-uniform
    const bool on = active;
    u64 fp = 0;
    bool have = false;
    const int qa = on ? S::quick_out_of_model(s, k, a.rt) : -1;
    if (qa >= 0) {      // generated, out of the model, no invariant to check: counted only
      ++nsucc;
      atomicAdd(&lds_cnt[qa], 1u);
    } else if (on) {
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
          have = fingerprint(t, fp);
          if (step_bad) { const u64 e = ev_word(gid, (u32)k, EV_VIOLATION); ev = e < ev ? e : ev; }
        } else if (a.inv_oom && (step_bad || S::violated(t, a.rt.invariants & S::inv_frame(act)))) {
          // TLC checks invariants on out-of-model successors ([ext] switch (ii)); first in key order wins
          // (only those the action can change: the parent satisfies all of them, S::inv_frame)
          const u64 e = ev_word(gid, (u32)k, EV_VIOLATION);
          ev = e < ev ? e : ev;
        }
      }
    }
    append(have, fp, k);
  }
  if constexpr (KEND < S::NI) {
    // DuplicateMessage(m) / DropMessage(m) (raft_original.tla:442-449) for bag slot q, in instance
    // order, unrolled (q is a compile-time constant): the successor is the parent (allLogs' applied)
    // with one message count +-1 — the count field is the low CNTB bits of bag entry q, at the
    // compile-time bit offset BAG_OFF + q * ENTB of the packed state.  Every other constraint reads
    // what the parent already satisfies, so the successor is in the model iff BoundedMessages keeps
    // the new count in [MinMsgCount, MaxMsgCount]; no invariant reads the bag (S::inv_frame), so an
    // out-of-model one is only counted.  Its fingerprint re-mixes the one or two 64-bit words that
    // hold the field (FpBase::fp_add_bit): no apply, no pack.  (C2: 532M of the 1,348M generated
    // successors, 266M of the 590M in the model; orig_materialize_plain still re-derives the new
    // ones through S::apply.)  The per-action count is uniform over the wave: one ballot and one LDS
    // atomic per slot.
    const bool bounded = (a.rt.constraints & OC_BoundedMessages) != 0;
    static_for<0, 2 * S::MK>([&](auto qc) {
      constexpr int q = decltype(qc)::value;
      constexpr bool dup = q < S::MK;
      constexpr int slot = dup ? q : q - S::MK;
      constexpr int k = S::I_DUP + q;
      const typename S::BE ent = s.bag.v[slot];
      const bool on = active && ent != S::BEMPTY;
      const int c = S::ecount(ent) + (dup ? 1 : -1);
      bool have = false;
      u64 fp = 0;
      if (on) {
        ++nsucc;
        if (bounded && (c < a.rt.min_count || c > a.rt.max_count)) {
          // out of the model (S::quick_out_of_model): counted only
        } else if (c < -8 || c > 7) {
          err |= OE_CAP_COUNT;                              // the packed count field holds -8..7 (bag_add_at)
        } else {
          have = true;
          ++nin;
          fp = fb.template fp_add_bit<S::BAG_OFF + slot * S::ENTB>(bw, dup ? 1 : -1, a.seed);
        }
      }
      {
        const u64 om = __ballot(on);
        if (om && lane == __ffsll((unsigned long long)om) - 1)
          atomicAdd(&lds_cnt[dup ? OA_DuplicateMessage : OA_DropMessage], (unsigned)__popcll(om));
      }
      append(have, fp, k);
    });
  }
  if (active) {
    if (err & OE_EVAL_LOG_INDEX) { const u64 e = ev_word(gid, 0, EV_NEXT_ERROR); ev = e < ev ? e : ev; }
    if (nsucc == 0 && a.deadlock && !lead) { const u64 e = ev_word(gid, 0, EV_DEADLOCK); ev = e < ev ? e : ev; }
  }
  {   // leader-work parents to the chunk's list: one global atomic per wave
    const u64 lm = __ballot(lead);
    if (lm) {
      const int first = __ffsll((unsigned long long)lm) - 1;
      u32 base = 0;
      if (lane == first) base = (u32)atomicAdd(&a.ctr[K_LEAD], (unsigned long long)__popcll(lm));
      base = __shfl(base, first);
      if (lead) a.lead[base + (u32)__popcll(lm & ((1ull << lane) - 1ull))] = (u32)tid | (nsucc == 0 ? 0x80000000u : 0u);
    }
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

// The instances [LEAD_LO, LEAD_HI) of the chunk's leader-work parents (the list orig_generate wrote),
// one lane per parent on full waves: the same successor / constraint / count / pack / FP64 work as
// orig_generate, the in-model records appended to the parent's own wave region of its generate
// workgroup (global atomic on that wave's record count: the dedup kernels read whole regions, and
// record order inside a region is immaterial: the FIFO merge keeps the minimum key, the -workers N
// filter decides by key).
template <class S>
__global__ void __launch_bounds__(BS) __attribute__((amdgpu_waves_per_eu(S::LEAD_WAVES))) orig_generate_lead(GenArgs a) {
  using W = typename S::Work;
  constexpr int NW = S::NW, NWP = (S::NW + 3) & ~3;
  __shared__ unsigned int lds_cnt[OA_NACT + 1];
  for (int t = threadIdx.x; t < OA_NACT + 1; t += BS) lds_cnt[t] = 0;
  __syncthreads();
  const u64 n = a.ctr[K_LEAD];
  constexpr bool INC = NW <= 16;
  u32 err = 0, nin = 0;
  unsigned long long ev = ~0ull;
  // grid-stride with a wave-uniform trip count (every lane of a wave runs the same instance loop)
  for (u64 i0 = (u64)blockIdx.x * BS; i0 < n; i0 += (u64)gridDim.x * BS) {
    const u64 i = i0 + threadIdx.x;
    const bool active = i < n;
    const u32 ent = active ? a.lead[i] : 0u;
    const u64 p = ent & 0x7fffffffu;                 // chunk index of the parent
    const u64 gid = a.gid0 + p;
    W s;
    u64 al[S::AW];
    if (active) {
      u32 w[NWP];
      const uint4* src = reinterpret_cast<const uint4*>(a.states + (a.chunk_begin + p) * NWP);
#pragma unroll
      for (int q = 0; q < NWP / 4; ++q) { const uint4 v = src[q]; w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w; }
      S::unpack(w, s);
      S::all_logs_next(s, al);
    } else {
      S::init(s);
#pragma unroll
      for (int q = 0; q < S::AW; ++q) al[q] = 0;
    }
    u32 bw[INC ? NW : 1];
    FpBase<INC ? NW : 2> fb;
    bool al_same = true;   // allLogs' = allLogs: a successor equal to bw is the parent (orig_generate)
#pragma unroll
    for (int q = 0; q < S::AW; ++q) al_same &= al[q] == s.allLogs[q];
    if constexpr (INC) {
      W b = s;
#pragma unroll
      for (int q = 0; q < S::AW; ++q) b.allLogs[q] = al[q];
      S::pack(b, bw);
      fb.init(bw, a.seed);
    }
    const u32 blk = (u32)(p / BS), plane = (u32)(p % BS);
    const u64 wreg = (u64)blk * (BS * S::NI) + (u64)(plane >> 6) * (64 * S::NI);
    u32* wcnt = a.rcnt + blk * 4 + (plane >> 6);
    u32 nsucc = 0, perr = 0;
#pragma unroll 1
    for (int k = S::LEAD_LO; k < S::LEAD_HI; ++k) {
      if (!active) continue;
      W t;
      const int act = S::apply(s, k, t, perr);
      if (act < 0) continue;
#pragma unroll
      for (int q = 0; q < S::AW; ++q) t.allLogs[q] = al[q];
      ++nsucc;
      atomicAdd(&lds_cnt[act], 1u);
      const bool step_bad = action_step_violated<S>(s, t, k, act, a.rt);
      if (S::in_model(t, a.rt)) {
        ++nin;
        if (step_bad) { const u64 e = ev_word(gid, (u32)k, EV_VIOLATION); ev = e < ev ? e : ev; }
        u32 pw[NW];
        S::pack(t, pw);
        u64 fp;
        if constexpr (INC) {
          bool changed;   // AdvanceCommitIndex(i) without an advance is its parent: no record
          fp = fb.fp(pw, bw, a.seed, changed);
          if (!changed && al_same) continue;
        } else {
          fp = fp64(pw, a.seed);
        }
        const u32 idx = atomicAdd(wcnt, 1u);
        a.rfp[wreg + idx] = fp;
        a.rkey[wreg + idx] = (unsigned short)((plane << 8) | (unsigned)k);
      } else if (a.inv_oom && (step_bad || S::violated(t, a.rt.invariants & S::inv_frame(act)))) {
        const u64 e = ev_word(gid, (u32)k, EV_VIOLATION);
        ev = e < ev ? e : ev;
      }
    }
    if (active) {
      if (perr & OE_EVAL_LOG_INDEX) { const u64 e = ev_word(gid, 0, EV_NEXT_ERROR); ev = e < ev ? e : ev; }
      if ((ent >> 31) && nsucc == 0 && a.deadlock) { const u64 e = ev_word(gid, 0, EV_DEADLOCK); ev = e < ev ? e : ev; }
      const u32 ce = perr & ~(u32)OE_EVAL_LOG_INDEX;
      if (ce) { atomicCAS(&a.ctr[K_ERRGID], 0ull, (unsigned long long)(gid + 1)); err |= ce; }
    }
  }
  if (err) atomicOr(&a.ctr[K_ERR], (unsigned long long)err);
  if (ev != ~0ull) atomicMin(&a.ctr[K_EVENT], ev);
  if (nin) atomicAdd(&lds_cnt[OA_NACT], nin);
  __syncthreads();
  for (int t = threadIdx.x; t < OA_NACT; t += BS)
    if (lds_cnt[t]) atomicAdd(&a.ctr[K_ACT + t], (unsigned long long)lds_cnt[t]);
  if (threadIdx.x == 0 && lds_cnt[OA_NACT]) atomicAdd(&a.ctr[K_GEN_IN], (unsigned long long)lds_cnt[OA_NACT]);
}

// Record i of workgroup b's four wave regions (concatenated in wave order): its offset in the
// workgroup's record region.  rc: the four per-wave counts; wreg = 64 * NI.
struct WaveRegions {
  u32 p1, p2, p3, n;
  u64 wreg;
  RMC_HD WaveRegions(const u32* rc, u64 wave_region) {
    p1 = rc[0]; p2 = p1 + rc[1]; p3 = p2 + rc[2]; n = p3 + rc[3]; wreg = wave_region;
  }
  RMC_HD u64 at(u32 i) const {
    const u32 w = (i >= p1) + (i >= p2) + (i >= p3);
    const u32 base = w == 0 ? 0u : w == 1 ? p1 : w == 2 ? p2 : p3;
    return (u64)w * wreg + (i - base);
  }
};

// Workgroup-local first-come fingerprint filter: answers only "certainly produced here before"
// (a full probe window lets the record through: the seen-set decides).  An empty slot is claimed
// by LDS CAS, so the set is exact up to the window: with plain stores (the round-4
// form) two lanes inserting different fingerprints into one slot at once left one of them out of
// the set, and two lanes with the same fingerprint both passed.  Measured on C2 (round 5,
// profiles/r05_dedup_ab.txt): 339.5M seen-set probes per run instead of 367.0M, orig_dedup_plain
// 11.30 vs 11.51 ms; a 16-slot window changed nothing (366.5M: overflow is not the leak) and an
// 8192-slot set (64 KB) cost occupancy (14.96 ms).
constexpr int LDS_WIN = 8;   // probe window of the LDS filter
template <int SLOTS = LDS_FP_SLOTS>
__device__ __forceinline__ bool lds_first(unsigned long long* set, u64 fp) {
  u32 h = (u32)(fp >> 20) & (SLOTS - 1);
#pragma unroll 1
  for (int p = 0; p < LDS_WIN; ++p) {
    unsigned long long cur = set[h];
    if (cur == fp) return false;            // produced here before
    if (cur == 0ull) {                      // claim the slot; a lane that loses the race looks at the winner's fp
      cur = atomicCAS(&set[h], 0ull, (unsigned long long)fp);
      if (cur == 0ull) return true;
      if (cur == fp) return false;
    }
    h = (h + 1) & (SLOTS - 1);
  }
  return true;                              // window full: let the seen-set decide
}

// ------------------------------------------------------------------ seen-set probing
// The seen-set: 2^k entries of 16 B {fp, ~key} (0 = empty), linear probing.  probe_batch inserts
// or finds G fingerprints at once (independent probes in flight), then lowers each entry's key
// to the given one (atomicMax of the complement; a key only ever decreases, so an entry that
// already holds a smaller key needs no atomic: the common case, a duplicate of an older state).
// ins bit j = this call inserted fp[j]; pos[j] = its entry index.
template <int G, bool KEYED = true, int STRIDE = 2>
__device__ __forceinline__ u32 probe_batch(u64* table, u64 mask, const u64 (&fp)[G], const u64 (&nk)[G], u64 (&pos)[G], u32& err) {
  static_assert(!KEYED || STRIDE == 2, "keyed entries are {fp, ~key}");
  u64 cur[G], cnk[G];
#pragma unroll
  for (int j = 0; j < G; ++j) {
    pos[j] = fp[j] & mask;
    if (fp[j] && KEYED) {
      const ulonglong2 e = *reinterpret_cast<const ulonglong2*>(table + 2 * pos[j]);
      cur[j] = e.x; cnk[j] = e.y;
    } else {
      cur[j] = fp[j] ? table[STRIDE * pos[j]] : ~0ull; cnk[j] = ~0ull;
    }
  }
  u32 ins = 0, lower = 0;
#pragma unroll
  for (int j = 0; j < G; ++j)
    if (fp[j] && cur[j] == 0ull) {
      cur[j] = (u64)atomicCAS((unsigned long long*)&table[STRIDE * pos[j]], 0ull, (unsigned long long)fp[j]);
      if (cur[j] == 0ull) { ins |= 1u << j; lower |= 1u << j; }
      else if (cur[j] == fp[j]) lower |= 1u << j;     // raced with another inserter of the same fp
    }
#pragma unroll
  for (int j = 0; j < G; ++j) {
    if (!fp[j] || ((lower >> j) & 1u)) continue;
    if (cur[j] == fp[j]) { if (KEYED && cnk[j] < nk[j]) lower |= 1u << j; continue; }
    u64 slot = (pos[j] + 1) & mask;
    for (u64 probe = 0;; ++probe) {
      if (probe > mask || probe >= (1u << 20)) { err |= OE_TABLE_FULL; break; }   // visited every entry
      u64 c, ck = ~0ull;
      if (KEYED) { const ulonglong2 e = *reinterpret_cast<const ulonglong2*>(table + 2 * slot); c = e.x; ck = e.y; }
      else c = table[STRIDE * slot];
      if (c == fp[j]) { if (KEYED && ck < nk[j]) lower |= 1u << j; break; }
      if (c == 0ull) {
        const u64 old = (u64)atomicCAS((unsigned long long*)&table[STRIDE * slot], 0ull, (unsigned long long)fp[j]);
        if (old == 0ull) { ins |= 1u << j; lower |= 1u << j; break; }
        if (old == fp[j]) { lower |= 1u << j; break; }
      }
      slot = (slot + 1) & mask;
    }
    pos[j] = slot;
  }
  if (KEYED) {
#pragma unroll
    for (int j = 0; j < G; ++j)
      if ((lower >> j) & 1u) atomicMax((unsigned long long*)&table[2 * pos[j] + 1], (unsigned long long)nk[j]);
  }
  return ins;
}

// one workgroup-wide exclusive scan of per-thread counts; returns this thread's offset, *total
__device__ __forceinline__ u32 block_excl_scan(u32 mine, u32* wave_tot, u32* total) {
  const int lane = __lane_id(), wave = threadIdx.x >> 6;
  u32 incl = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const u32 v = __shfl_up(incl, d); if (lane >= d) incl += v; }
  if (lane == 63) wave_tot[wave] = incl;
  __syncthreads();
  u32 base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < BS / 64; ++w) { const u32 x = wave_tot[w]; if (w < wave) base += x; tot += x; }
  *total = tot;
  __syncthreads();   // wave_tot may be reused
  return base + incl - mine;
}

struct DedupArgs {
  const u64* rfp;
  const unsigned short* rkey;
  const u32* rcnt;
  u64 region;                  // records per workgroup region (BS * NI)
  u64 gid0;                    // global id of the chunk's first parent
  ulonglong2* urec;            // [nblk][region] distinct (fp, ~key) of each workgroup's records
  u32* ucnt;                   // [nblk]
  u64* table;
  u64 table_mask;
  u64* newpos;                 // entry indices inserted by this chunk (ctr[K_INS] of them)
  unsigned long long* ctr;
  u32 prof;                    // accumulate per-workgroup wall-clock ticks into ctr[K_PROF..]
};

RMC_HD u64 nkey_of(u64 gid0, u32 blk, u32 lk) {   // ~(global key) of a local record key
  return ~(((gid0 + (u64)blk * BS + (lk >> 8)) << 8) | (u64)(lk & 255u));
}

// insert-or-find fp in the workgroup's LDS set and lower its slot's key to lk; false = window full
__device__ __forceinline__ bool lds_merge(unsigned long long* lfp, unsigned int* lkey, u64 fp, u32 lk) {
  u32 h = (u32)(fp >> 20) & (LDS_FP_SLOTS - 1);
#pragma unroll 1
  for (int p = 0; p < 8; ++p) {
    unsigned long long c = lfp[h];                                   // plain read first: most hits need no CAS
    if (c == 0ull) c = atomicCAS(&lfp[h], 0ull, (unsigned long long)fp);
    if (c == 0ull || c == fp) { atomicMin(&lkey[h], lk); return true; }
    h = (h + 1) & (LDS_FP_SLOTS - 1);
  }
  return false;
}

// Seen-set insertion, part 1 (LDS): workgroup b takes generate-workgroup b's records and merges
// them in an LDS set {fp, min local key} (exact: LDS CAS + LDS atomicMin; ~half of C2's
// successors repeat another successor of the same 256 parents).  The distinct (fp, ~global key)
// pairs are written compacted to the workgroup's region (a record whose probe window is full
// goes there with its own key: the seen-set keeps the minimum key anyway).  Splitting the merge
// from the probes lets the probe kernel run at the occupancy its registers allow, instead of
// the 3 workgroups per CU the 48-KB set allows (measured: fused merge + probes 17-21 ms of C2).
__global__ void __launch_bounds__(BS) orig_merge(DedupArgs a) {
  __shared__ unsigned long long lfp[LDS_FP_SLOTS];
  __shared__ unsigned int lkey[LDS_FP_SLOTS];
  __shared__ u32 wave_tot[BS / 64];
  __shared__ u32 ovf_cnt;
  for (int t = threadIdx.x; t < LDS_FP_SLOTS; t += BS) { lfp[t] = 0ull; lkey[t] = ~0u; }
  if (threadIdx.x == 0) ovf_cnt = 0;
  __syncthreads();
  const WaveRegions wr(a.rcnt + 4 * blockIdx.x, a.region / 4);
  const u32 n = wr.n;
  const u64* fps = a.rfp + (u64)blockIdx.x * a.region;
  const unsigned short* keys = a.rkey + (u64)blockIdx.x * a.region;
  ulonglong2* out = a.urec + (u64)blockIdx.x * a.region;
  // overflow records (probe window full) go to the END of the region, growing down
  constexpr int P1 = 8;
#pragma unroll 1
  for (u32 i0 = 0; i0 < n; i0 += P1 * BS) {
    u64 fp[P1];
    u32 lk[P1];
#pragma unroll
    for (int j = 0; j < P1; ++j) {
      const u32 i = i0 + (u32)j * BS + threadIdx.x;
      const u64 at = wr.at(i);
      fp[j] = i < n ? fps[at] : 0ull;
      lk[j] = i < n ? (u32)keys[at] : 0u;
    }
#pragma unroll
    for (int j = 0; j < P1; ++j) {
      if (fp[j] && !lds_merge(lfp, lkey, fp[j], lk[j])) {   // window full (rare): the record keeps its own key
        const u32 at = atomicAdd(&ovf_cnt, 1u);
        out[a.region - 1 - at] = make_ulonglong2((unsigned long long)fp[j], (unsigned long long)nkey_of(a.gid0, blockIdx.x, lk[j]));
      }
    }
  }
  __syncthreads();
  // compact the set's occupied slots to the front of the region
  constexpr int PER = LDS_FP_SLOTS / BS;
  u32 mine = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) mine += lfp[threadIdx.x * PER + j] ? 1u : 0u;
  u32 total = 0;
  u32 o = block_excl_scan(mine, wave_tot, &total);
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int sl = threadIdx.x * PER + j;
    const u64 fp = lfp[sl];
    if (fp) out[o++] = make_ulonglong2((unsigned long long)fp, (unsigned long long)nkey_of(a.gid0, blockIdx.x, lkey[sl]));
  }
  const u32 nov = ovf_cnt;   // (read after the scan's barriers)
  __syncthreads();
  // move the overflow records (end of the region) behind the set's.  Their order is free, so when the
  // two runs meet (total + 2 * nov > region: a region filled by records of few LDS windows) only the
  // records beyond total + nov move, into the gap below the run: sources and destinations never
  // overlap, whichever thread runs first.  (Moving all nov of them let one thread overwrite a record
  // that another had yet to read, which lost fingerprints.)
  const u32 gap = (u32)a.region - total - nov;
  const u32 mv = nov < gap ? nov : gap;
  for (u32 q = threadIdx.x; q < mv; q += BS) out[total + q] = out[a.region - 1 - q];
  if (threadIdx.x == 0) a.ucnt[blockIdx.x] = total + nov;
}

// Seen-set insertion, part 2 (HBM random access): workgroup b probes the seen-set once per
// distinct fingerprint of region b, DEDUP_PER probes in flight per thread (insert-if-absent by CAS
// of the fp, then atomicMax of ~key: the entry keeps the minimum key), and appends the inserted
// entries' positions (one global atomic per workgroup and round).  COUNT: also count the probes
// (ctr[K_PROBES]; RAFTMC_COUNT_PROBES, a run of its own: timed runs leave the atomic out)
template <bool COUNT>
__global__ void __launch_bounds__(BS) orig_probe(DedupArgs a) {
  __shared__ u32 wave_tot[BS / 64];
  __shared__ unsigned long long base_sh;
  const u32 n = a.ucnt[blockIdx.x];
  const ulonglong2* in = a.urec + (u64)blockIdx.x * a.region;
  u32 err = 0;
  const u64 t0 = a.prof ? wall_clock64() : 0;
  if (COUNT && threadIdx.x == 0 && n) atomicAdd(&a.ctr[K_PROBES], (unsigned long long)n);
#pragma unroll 1
  for (u32 i0 = 0; i0 < n; i0 += DEDUP_PER * BS) {
    u64 fp[DEDUP_PER], nk[DEDUP_PER], pos[DEDUP_PER];
#pragma unroll
    for (int j = 0; j < DEDUP_PER; ++j) {
      const u32 i = i0 + (u32)j * BS + threadIdx.x;
      const ulonglong2 r = i < n ? in[i] : make_ulonglong2(0ull, 0ull);
      fp[j] = r.x; nk[j] = r.y;
    }
    const u32 ins = probe_batch<DEDUP_PER>(a.table, a.table_mask, fp, nk, pos, err);
    u32 total = 0;
    const u32 off = block_excl_scan((u32)__popc(ins), wave_tot, &total);
    if (threadIdx.x == 0) base_sh = total ? atomicAdd(&a.ctr[K_INS], (unsigned long long)total) : 0ull;
    __syncthreads();
    u64 o = base_sh + off;
#pragma unroll
    for (int j = 0; j < DEDUP_PER; ++j)
      if ((ins >> j) & 1u) a.newpos[o++] = pos[j];
    __syncthreads();   // base_sh reused
  }
  if (err) atomicOr(&a.ctr[K_ERR], (unsigned long long)err);
  if (a.prof && threadIdx.x == 0) {
    const u64 t3 = wall_clock64();
    atomicAdd(&a.ctr[K_PROF + 1], (unsigned long long)(t3 - t0));
    atomicAdd(&a.ctr[K_PROF + 3], 1ull);
  }
}

// ------------------------------------------------------------------ TLC -workers N semantics
// The order-independent pipeline (mc_opts.workers != 1): every count TLC prints without -coverage
// is the same, but which producer of a state is kept is not TLC's single-worker choice (as with
// TLC's own workers).  8-B seen-set entries, first-come LDS filter, no keys, no winner pass: the
// inserting thread numbers its new state directly.

// Fused variant for TLC -workers N (what the pipeline runs): records through a first-come LDS
// filter (lds_first: an LDS CAS claims each empty slot, 8 B per slot; a full window lets a record through to
// the seen-set, never drop a state), the survivors probe the 8-B seen-set PER at a time, and
// the new states' producers go out parent-major (an LDS winner mask per parent).  PER, SLOTS: DEDUP_PER and
// LDS_FP_SLOTS on a launch of its own, OVERLAP_DEDUP_PER and OVERLAP_LDS_FP_SLOTS beside a generate
// (launch_dedup_plain); DYN: the filter is the launch's dynamic LDS (SLOTS * 8 B), not a static array
// (OVERLAP_DEDUP_PER's comment).  COUNT: also count the
// fingerprints that reach the seen-set (ctr[K_PROBES], one atomic per workgroup) -- a separate
// instantiation, because even one extra same-address atomic per wave costs ~3 ms of C2's
// 11 ms here (round 4, measured), so timed runs leave it off (RAFTMC_COUNT_PROBES).
template <int WW, bool COUNT, int PER = DEDUP_PER, int SLOTS = LDS_FP_SLOTS, bool DYN = false>
__global__ void __launch_bounds__(BS) orig_dedup_plain(DedupArgs a) {
  __shared__ unsigned long long lfp_static[DYN ? 1 : SLOTS];
  extern __shared__ unsigned long long lfp_dynamic[];
  unsigned long long* const lfp = DYN ? lfp_dynamic : lfp_static;
  __shared__ u32 wave_tot[BS / 64];
  __shared__ unsigned long long base_sh;
  __shared__ unsigned long long win[BS * WW];
  for (int t = threadIdx.x; t < SLOTS; t += BS) lfp[t] = 0ull;
  for (int t = threadIdx.x; t < BS * WW; t += BS) win[t] = 0ull;
  __syncthreads();
  const WaveRegions wr(a.rcnt + 4 * blockIdx.x, a.region / 4);
  const u32 n = wr.n;
  const u64* fps = a.rfp + (u64)blockIdx.x * a.region;
  const unsigned short* keys = a.rkey + (u64)blockIdx.x * a.region;
  u32 err = 0;
  u32 probes = 0;   // this lane's (summed over the wave at the end)
#pragma unroll 1
  for (u32 i0 = 0; i0 < n; i0 += PER * BS) {
    u64 fp[PER], key[PER], pos[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const u32 i = i0 + (u32)j * BS + threadIdx.x;
      const u64 at = wr.at(i);
      fp[j] = i < n ? fps[at] : 0ull;
      key[j] = i < n ? (u64)keys[at] : 0ull;     // local key lane << 8 | instance
    }
#pragma unroll
    for (int j = 0; j < PER; ++j)
      if (fp[j] && !lds_first<SLOTS>(lfp, fp[j])) fp[j] = 0ull;   // produced by this workgroup's parents before
    if constexpr (COUNT) {
#pragma unroll
      for (int j = 0; j < PER; ++j) probes += fp[j] ? 1u : 0u;
    }
    const u32 ins = probe_batch<PER, false, 1>(a.table, a.table_mask, fp, key, pos, err);
#pragma unroll
    for (int j = 0; j < PER; ++j)
      if ((ins >> j) & 1u) atomicOr(&win[(key[j] >> 8) * WW + ((key[j] & 255) >> 6)], 1ull << (key[j] & 63));
  }
  __shared__ u32 wave_probes[BS / 64];
  if constexpr (COUNT) {
    u32 wp = probes;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) wp += __shfl_xor(wp, d);
    if (__lane_id() == 0) wave_probes[threadIdx.x >> 6] = wp;
  }
  __syncthreads();
  if constexpr (COUNT) {
    if (threadIdx.x == 0) {
      u32 t = 0;
#pragma unroll
      for (int w = 0; w < BS / 64; ++w) t += wave_probes[w];
      if (t) atomicAdd(&a.ctr[K_PROBES], (unsigned long long)t);
    }
  }
  u64 wm[WW];
  u32 mine = 0;
#pragma unroll
  for (int q = 0; q < WW; ++q) { wm[q] = win[threadIdx.x * WW + q]; mine += (u32)__popcll(wm[q]); }
  u32 total = 0;
  const u32 off = block_excl_scan(mine, wave_tot, &total);
  if (threadIdx.x == 0) base_sh = total ? atomicAdd(&a.ctr[K_CHUNK_NEW], (unsigned long long)total) : 0ull;
  __syncthreads();
  u64 o = base_sh + off;
  const u64 pg = a.gid0 + (u64)blockIdx.x * BS + threadIdx.x;
#pragma unroll
  for (int q = 0; q < WW; ++q) {
    u64 m = wm[q];
    while (m) {
      const int k = q * 64 + __ffsll((unsigned long long)m) - 1;
      m &= m - 1;
      a.newpos[o++] = (pg << 8) | (u64)k;
    }
  }
  if (err) atomicOr(&a.ctr[K_ERR], (unsigned long long)err);
}

struct MatPlainArgs {
  u32* states;
  u64* meta;
  const u64* newrec;           // (parent gid << 8 | instance), ctr[K_CHUNK_NEW] of them
  u64 base;                    // global id of device slot 0
  u64 dst_base, cap;           // new state i of the chunk goes to dst_base + ctr[K_LEVEL_NEW] + i (device index)
  OrigRuntime rt;
  unsigned long long* ctr;
  u32 store;                   // 0: the last level of a depth-bounded search (count_final_level):
                               // counted and invariant-checked, not written
};

// grid-stride over the chunk's new states (their count stays on the device: no host wait)
template <class S>
__global__ void __launch_bounds__(BS) orig_materialize_plain(MatPlainArgs a) {
  using W = typename S::Work;
  constexpr int NW = S::NW, NWP = (S::NW + 3) & ~3;
  __shared__ unsigned int lds_cnt[OA_NACT];
  for (int t = threadIdx.x; t < OA_NACT; t += BS) lds_cnt[t] = 0;
  __syncthreads();
  const u64 n_new = a.ctr[K_CHUNK_NEW];
  const u64 base = a.dst_base + a.ctr[K_LEVEL_NEW];
  u32 err = 0;
  unsigned long long ev = ~0ull;
  for (u64 i = (u64)blockIdx.x * BS + threadIdx.x; i < n_new; i += (u64)gridDim.x * BS) {
    const u64 rec = a.newrec[i], pgid = rec >> 8;
    const int k = (int)(rec & 0xff);
    u32 w[NWP];
    const uint4* src = reinterpret_cast<const uint4*>(a.states + (pgid - a.base) * NWP);
#pragma unroll
    for (int q = 0; q < NWP / 4; ++q) { const uint4 v = src[q]; w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w; }
    W s, t;
    u64 al[S::AW];
    S::unpack(w, s);
    S::all_logs_next(s, al);
    u32 e2 = 0;
    const int act = S::apply(s, k, t, e2);
#pragma unroll
    for (int q = 0; q < S::AW; ++q) t.allLogs[q] = al[q];
    u32 pw[NW];
    S::pack(t, pw);
    const u64 dst = base + i;
    if (act >= 0 && (!a.store || dst < a.cap)) {
      if (a.store) {
        uint4* o = reinterpret_cast<uint4*>(a.states + dst * NWP);
#pragma unroll
        for (int q = 0; q < NWP / 4; ++q)
          o[q] = make_uint4(pw[4 * q], 4 * q + 1 < NW ? pw[4 * q + 1] : 0u, 4 * q + 2 < NW ? pw[4 * q + 2] : 0u, 4 * q + 3 < NW ? pw[4 * q + 3] : 0u);
        a.meta[dst] = (pgid << 24) | ((u64)act << 16) | (u64)k;
      }
      atomicAdd(&lds_cnt[act], 1u);
      if (S::violated(t, a.rt.invariants & S::inv_frame(act))) { const u64 e = ev_word(pgid, (u32)k, EV_VIOLATION); ev = e < ev ? e : ev; }
    } else {
      err |= dst >= a.cap ? (u32)OE_CAP_STORE : (u32)OE_TABLE_FULL;
    }
  }
  if (err) atomicOr(&a.ctr[K_ERR], (unsigned long long)err);
  if (ev != ~0ull) atomicMin(&a.ctr[K_EVENT], ev);
  __syncthreads();
  for (int t = threadIdx.x; t < OA_NACT; t += BS)
    if (lds_cnt[t]) atomicAdd(&a.ctr[K_ACT + OA_NACT + t], (unsigned long long)lds_cnt[t]);
}

// Winners: an entry inserted by this chunk holds, after the chunk's dedup, the minimum key over
// all its producers (later chunks have larger keys), i.e. TLC's first-found (parent, instance).
// orig_mark sets that (parent, instance) bit; orig_count counts each workgroup's winners.
struct MarkArgs {
  const u64* newpos;
  const u64* table;
  u64 gid0, chunk_count;
  u64* winmask;                // [chunk][WW] instance bits of each parent's winning successors
  u32 ww;
  unsigned long long* ctr;
};

__global__ void __launch_bounds__(BS) orig_mark(MarkArgs a) {
  const u64 n = a.ctr[K_INS];
  for (u64 i = (u64)blockIdx.x * BS + threadIdx.x; i < n; i += (u64)gridDim.x * BS) {
    const u64 key = ~a.table[2 * a.newpos[i] + 1];
    const u64 p = (key >> 8) - a.gid0;
    const u32 k = (u32)(key & 255);
    if (p >= a.chunk_count) { atomicOr(&a.ctr[K_ERR], (unsigned long long)OE_TABLE_FULL); continue; }   // cannot happen
    atomicOr((unsigned long long*)&a.winmask[p * a.ww + (k >> 6)], 1ull << (k & 63));
  }
}

// winners per workgroup of 256 parents (popcount of their masks; coalesced, no atomics)
template <int WW>
__global__ void __launch_bounds__(BS) orig_count(const u64* winmask, u64 chunk_count, u32* wcnt) {
  __shared__ u32 wave_tot[BS / 64];
  const u64 p = (u64)blockIdx.x * BS + threadIdx.x;
  u32 mine = 0;
#pragma unroll
  for (int q = 0; q < WW; ++q) mine += p < chunk_count ? (u32)__popcll(winmask[p * WW + q]) : 0u;
  u32 total = 0;
  (void)block_excl_scan(mine, wave_tot, &total);
  if (threadIdx.x == 0) wcnt[blockIdx.x] = total;
}

// exclusive scan of the per-workgroup winner counts -> woff; the chunk's total -> ctr[K_CHUNK_NEW]
__global__ void __launch_bounds__(SCAN_BS) orig_scan(const u32* wcnt, u64* woff, u32 nblk, unsigned long long* ctr) {
  __shared__ unsigned long long part[SCAN_BS];
  const u32 per = (nblk + SCAN_BS - 1) / SCAN_BS, b0 = threadIdx.x * per;
  unsigned long long s = 0;
  for (u32 j = 0; j < per; ++j) if (b0 + j < nblk) s += wcnt[b0 + j];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int d = 1; d < SCAN_BS; d <<= 1) {
    const unsigned long long x = threadIdx.x >= (unsigned)d ? part[threadIdx.x - d] : 0ull;
    __syncthreads();
    part[threadIdx.x] += x;
    __syncthreads();
  }
  unsigned long long run = part[threadIdx.x] - s;
  for (u32 j = 0; j < per; ++j) if (b0 + j < nblk) { woff[b0 + j] = run; run += wcnt[b0 + j]; }
  if (threadIdx.x == SCAN_BS - 1) ctr[K_CHUNK_NEW] = part[SCAN_BS - 1];
}

struct MatArgs {
  u32* states;
  u64* meta;
  u64 chunk_begin, chunk_count, gid0;   // parents: device index, count, global id of the first
  u64* winmask;                // read and re-zeroed
  const u64* woff;
  u32 ww;
  u64 dst_base, cap;           // new state i of the chunk goes to dst_base + ctr[K_LEVEL_NEW] + i (device index)
  OrigRuntime rt;
  unsigned long long* ctr;
};

// Workgroup per 256 parents (the generate workgroup's): the winners in key order — parent
// order, then instance order — are numbered by a workgroup scan plus the chunk offset, staged
// in LDS and spread over the workgroup's lanes; each is re-derived from (parent, instance) and
// stored at its FIFO position with its parent pointer; invariants of the new state.
template <class S>
__global__ void __launch_bounds__(BS) orig_materialize(MatArgs a) {
  using W = typename S::Work;
  constexpr int NW = S::NW, NWP = (S::NW + 3) & ~3, WW = (S::NI + 63) / 64;
  __shared__ unsigned int lds_cnt[OA_NACT];
  __shared__ unsigned short items[MAT_CAP];
  __shared__ u32 wave_tot[BS / 64];
  for (int t = threadIdx.x; t < OA_NACT; t += BS) lds_cnt[t] = 0;
  const u64 p = (u64)blockIdx.x * BS + threadIdx.x;
  u64 wm[WW];
  u32 mine = 0;
#pragma unroll
  for (int q = 0; q < WW; ++q) {
    wm[q] = p < a.chunk_count ? a.winmask[p * WW + q] : 0ull;
    mine += (u32)__popcll(wm[q]);
  }
  if (p < a.chunk_count && mine) {
#pragma unroll
    for (int q = 0; q < WW; ++q) a.winmask[p * WW + q] = 0ull;   // ready for the next chunk
  }
  u32 total = 0;
  const u32 off = block_excl_scan(mine, wave_tot, &total);   // (also orders lds_cnt's clearing)
  const u64 base = a.dst_base + a.ctr[K_LEVEL_NEW] + a.woff[blockIdx.x];
  u32 err = 0;
  unsigned long long ev = ~0ull;
  for (u32 r0 = 0; r0 < total; r0 += MAT_CAP) {
    {   // stage this round's window [r0, r0 + MAT_CAP) of the workgroup's winners
      u32 idx = off;
#pragma unroll
      for (int q = 0; q < WW; ++q) {
        u64 m = wm[q];
        while (m) {
          const int k = q * 64 + __ffsll((unsigned long long)m) - 1;
          m &= m - 1;
          if (idx >= r0 && idx < r0 + MAT_CAP) items[idx - r0] = (unsigned short)((threadIdx.x << 8) | (unsigned)k);
          ++idx;
        }
      }
    }
    __syncthreads();
    const u32 nr = total - r0 < (u32)MAT_CAP ? total - r0 : (u32)MAT_CAP;
    for (u32 i = threadIdx.x; i < nr; i += BS) {
      const u32 x = items[i];
      const u64 par = (u64)blockIdx.x * BS + (x >> 8);
      const int k = (int)(x & 255);
      u32 w[NWP];
      const uint4* src = reinterpret_cast<const uint4*>(a.states + (a.chunk_begin + par) * NWP);
#pragma unroll
      for (int q = 0; q < NWP / 4; ++q) { const uint4 v = src[q]; w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w; }
      W s, t;
      u64 al[S::AW];
      S::unpack(w, s);
      S::all_logs_next(s, al);
      u32 e2 = 0;
      const int act = S::apply(s, k, t, e2);
#pragma unroll
      for (int q = 0; q < S::AW; ++q) t.allLogs[q] = al[q];
      u32 pw[NW];
      S::pack(t, pw);
      const u64 dst = base + r0 + i;
      if (act >= 0 && dst < a.cap) {
        uint4* o = reinterpret_cast<uint4*>(a.states + dst * NWP);
#pragma unroll
        for (int q = 0; q < NWP / 4; ++q)
          o[q] = make_uint4(pw[4 * q], 4 * q + 1 < NW ? pw[4 * q + 1] : 0u, 4 * q + 2 < NW ? pw[4 * q + 2] : 0u, 4 * q + 3 < NW ? pw[4 * q + 3] : 0u);
        const u64 pgid = a.gid0 + par;
        a.meta[dst] = (pgid << 24) | ((u64)act << 16) | (u64)k;
        atomicAdd(&lds_cnt[act], 1u);
        if (S::violated(t, a.rt.invariants & S::inv_frame(act))) {
          const u64 e = ev_word(pgid, (u32)k, EV_VIOLATION);
          ev = e < ev ? e : ev;
        }
      } else {
        err |= dst >= a.cap ? (u32)OE_CAP_STORE : (u32)OE_TABLE_FULL;   // a winner always re-derives
      }
    }
    __syncthreads();
  }
  if (err) atomicOr(&a.ctr[K_ERR], (unsigned long long)err);
  if (ev != ~0ull) atomicMin(&a.ctr[K_EVENT], ev);
  __syncthreads();
  for (int t = threadIdx.x; t < OA_NACT; t += BS)
    if (lds_cnt[t]) atomicAdd(&a.ctr[K_ACT + OA_NACT + t], (unsigned long long)lds_cnt[t]);
}

// after a chunk's materialize: fold its new-state count into the level's; re-arm the chunk's
// insert counter (the level's first chunk starts from the per-level counter reset)
// (Vector atomics only: with plain accesses the compiler reads the counters with a scalar load
// and may issue the vector store that zeroes K_CHUNK_NEW before that load has returned — on the
// GPU the load then sometimes sees the zero and the chunk's new states are lost.  Found when a
// fourth counter store moved the scalar wait behind the stores.)
// rearm_lead = 0: a pipelined level (run(), "generate beside dedup"), whose generate stream re-arms
// K_LEAD itself -- zeroing it here would wipe the count of the next sub-chunk's orig_generate, which
// runs beside this kernel.
__global__ void orig_advance(unsigned long long* ctr, int rearm_lead) {
  if (threadIdx.x == 0) {
    const unsigned long long n = atomicExch(&ctr[K_CHUNK_NEW], 0ull);
    atomicAdd(&ctr[K_LEVEL_NEW], n);
    atomicExch(&ctr[K_INS], 0ull);
    if (rearm_lead) atomicExch(&ctr[K_LEAD], 0ull);
  }
}

// the level's counters back to their initial values (event word all ones); queued right after
// the level's counter readback, so it runs while the host looks at the counters and the next
// level starts with its generate kernel (one tiny kernel instead of two fills on the critical path)
__global__ void orig_reset_ctr(unsigned long long* ctr) {
  for (int t = threadIdx.x; t < K_NCTR; t += blockDim.x) ctr[t] = t == K_EVENT ? ~0ull : 0ull;
}

// level start behind a hoisted generate (run()): what orig_generate + orig_generate_lead
// of the level's first parents counted in their own block goes into the level's counters, and that
// block is back at orig_reset_ctr's values (its K_LEAD was the hoisted pair's alone).  The counters
// the generate kernels never touch are zero in ctr2 and stay out.  Vector atomics only, as in
// orig_advance.
__global__ void orig_fold_ctr(unsigned long long* ctr, unsigned long long* ctr2) {
  for (int t = threadIdx.x; t < K_NCTR; t += blockDim.x) {
    const unsigned long long v = atomicExch(&ctr2[t], t == K_EVENT ? ~0ull : 0ull);
    if (t == K_EVENT) atomicMin(&ctr[t], v);
    else if (t == K_ERR) atomicOr(&ctr[t], v);
    else if (t == K_ERRGID) { if (v) atomicCAS(&ctr[t], 0ull, v); }
    else if (t == K_GEN_IN || t == K_PROBES || (t >= K_ACT && t < K_ACT + OA_NACT)) atomicAdd(&ctr[t], v);
  }
}

// run start: the initial state (global id 0), its meta word (no parent) and its seen-set entry
// (key 0), written on the run's stream so that nothing at run start blocks the host
template <int NWP>
struct InitWords { u32 w[NWP]; };
template <int NWP, int STRIDE>
__global__ void orig_init_state(InitWords<NWP> s0, u32* states, u64* meta, u64* table, u64 mask, u64 fp) {
  if (threadIdx.x < NWP) states[threadIdx.x] = s0.w[threadIdx.x];
  if (threadIdx.x == 0) {
    meta[0] = ~0ull;
    const u64 pos = fp & mask;
    table[STRIDE * pos] = fp;
    if (STRIDE == 2) table[2 * pos + 1] = ~0ull;
  }
}

// The seen-set moves from the starter table to the (just cleared) full table: every occupied
// starter entry is inserted by linear probing with CAS.  Runs alone on the stream, between two
// levels; the starter holds each fingerprint once, so an inserted entry belongs to one lane and
// its ~key word (STRIDE 2: TLC's FIFO order) is a plain store.  moved (may be null): entries moved.
template <int STRIDE>
__global__ void __launch_bounds__(BS) orig_migrate(const u64* src, u64 n, u64* dst, u64 mask, unsigned long long* ctr,
                                                   unsigned long long* moved) {
  constexpr int E = 4 / STRIDE;   // entries per 32-B group: the walk is a stream of 16-B loads (n is a multiple of E)
  u32 mine = 0, err = 0;
#pragma unroll 2
  for (u64 g = (u64)blockIdx.x * BS + threadIdx.x; g < n / E; g += (u64)gridDim.x * BS) {
    const ulonglong2* p = reinterpret_cast<const ulonglong2*>(src + 4 * g);
    const ulonglong2 lo = p[0], hi = p[1];
    const u64 v[4] = {lo.x, lo.y, hi.x, hi.y};
#pragma unroll
    for (int j = 0; j < E; ++j) {
      const u64 fp = v[STRIDE * j], nk = STRIDE == 2 ? v[2 * j + 1] : 0ull;
      if (!fp) continue;
      ++mine;
      u64 slot = fp & mask;
      for (u64 probe = 0;; ++probe) {
        if (probe > mask || probe >= (1u << 20)) { err |= OE_TABLE_FULL; break; }   // as probe_batch
        if (dst[STRIDE * slot] == 0ull &&
            atomicCAS((unsigned long long*)&dst[STRIDE * slot], 0ull, (unsigned long long)fp) == 0ull) {
          if (STRIDE == 2) dst[2 * slot + 1] = nk;
          break;
        }
        slot = (slot + 1) & mask;
      }
    }
  }
  if (err) atomicOr(&ctr[K_ERR], (unsigned long long)err);
  if (moved) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d);
    if (__lane_id() == 0 && mine) atomicAdd(moved, (unsigned long long)mine);
  }
}

// ------------------------------------------------------------------ TLC's stop point
// On the level's first event (parent gid_stop, instance k_stop, kind): TLC's generated counts
// are the whole successor lists of the parents before it and of the event's parent (none when
// computing its successors raised the error), per-action generated counts stop at the event's
// successor.  out[0] = generated, out[1 + a] = per-action generated.
template <class S>
__global__ void __launch_bounds__(BS) orig_stop_generated(const u32* states, u64 first, u64 n, u64 gid0, u64 gid_stop,
                                                         u32 k_stop, u32 kind, unsigned long long* out) {
  using W = typename S::Work;
  constexpr int NWP = (S::NW + 3) & ~3;
  // counts in LDS, one global atomic per workgroup and action (a global atomic per successor on
  // 16 addresses serialises: minutes for C5v2's 93M-parent level 11)
  __shared__ unsigned int lds_cnt[1 + OA_NACT];
  for (int q = threadIdx.x; q < 1 + OA_NACT; q += BS) lds_cnt[q] = 0;
  __syncthreads();
  const u64 i = (u64)blockIdx.x * BS + threadIdx.x;
  const u64 gid = gid0 + i;
  if (i < n && !(gid == gid_stop && kind == EV_NEXT_ERROR)) {
    u32 w[NWP];
#pragma unroll
    for (int q = 0; q < NWP; ++q) w[q] = states[(first + i) * NWP + q];
    W s, t;
    S::unpack(w, s);
    u32 err = 0, tot = 0;
    for (int k = 0; k < S::NI; ++k) {
      const int act = S::apply(s, k, t, err);
      if (act < 0) continue;
      ++tot;
      if (gid < gid_stop || (u32)k <= k_stop) atomicAdd(&lds_cnt[1 + act], 1u);
    }
    if (tot) atomicAdd(&lds_cnt[0], tot);
  }
  __syncthreads();
  for (int q = threadIdx.x; q < 1 + OA_NACT; q += BS)
    if (lds_cnt[q]) atomicAdd(&out[q], (unsigned long long)lds_cnt[q]);
}

// per-action distinct counts of the level's first n new states (stored in key order)
__global__ void __launch_bounds__(BS) orig_stop_distinct(const u64* meta, u64 n, unsigned long long* out) {
  __shared__ unsigned int lds_cnt[OA_NACT];
  for (int q = threadIdx.x; q < OA_NACT; q += BS) lds_cnt[q] = 0;
  __syncthreads();
  const u64 i = (u64)blockIdx.x * BS + threadIdx.x;
  if (i < n) atomicAdd(&lds_cnt[((meta[i] >> 16) & 0xff) % OA_NACT], 1u);
  __syncthreads();
  for (int q = threadIdx.x; q < OA_NACT; q += BS)
    if (lds_cnt[q]) atomicAdd(&out[q], (unsigned long long)lds_cnt[q]);
}

// ------------------------------------------------------------------ sharded (multi-GPU) kernels
// owner of a fingerprint: high half mod world (the seen-set index uses the low bits)
__device__ __host__ __forceinline__ u32 fp_owner(u64 fp, u32 world) { return (u32)((fp >> 32) % world); }

struct RouteArgs {
  const u64* rfp;
  const unsigned short* rkey;
  const u32* rcnt;
  u64 region;                  // records per workgroup region (BS * NI)
  u64* route;                  // [world][route_cap][2] (fp, slot)
  u64 route_cap;
  u32 world;
  unsigned long long* rcnt_out;   // [world]
};

// Sharded route over the compacted records: workgroup b takes generate-workgroup b's records,
// drops the successors its 256 parents produce more than once (the first-come LDS filter), and
// buckets the rest by owner, 16 records per thread at a time: LDS histogram, one global atomic
// per (workgroup, round, owner).  Records are (fp, state in chunk << 8 | instance).
// (its filter keeps 4096 slots: the route kernel's 16 records per thread make it VGPR-bound, so the
// larger set costs no occupancy here and saves the stores it filters: 7.1 vs 8.0 ms per C2 run at world 1)
constexpr int ROUTE_FP_SLOTS = 4096;
__global__ void __launch_bounds__(BS) orig_route_blk(RouteArgs a) {
  __shared__ unsigned long long lds_fp[ROUTE_FP_SLOTS];
  __shared__ unsigned int hist[8];
  __shared__ unsigned long long base[8];
  for (int t = threadIdx.x; t < ROUTE_FP_SLOTS; t += BS) lds_fp[t] = 0ull;
  const WaveRegions wr(a.rcnt + 4 * blockIdx.x, a.region / 4);
  const u32 n = wr.n;
  const u64* fps = a.rfp + (u64)blockIdx.x * a.region;
  const unsigned short* keys = a.rkey + (u64)blockIdx.x * a.region;
  constexpr int G = 16;
#pragma unroll 1
  for (u32 i0 = 0; i0 < n; i0 += G * BS) {
    if (threadIdx.x < 8) hist[threadIdx.x] = 0;
    __syncthreads();   // also orders the set's clearing before its first use
    u64 fp[G], slot[G];
    unsigned int off[G];
    int own[G];
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const u32 i = i0 + (u32)j * BS + threadIdx.x;
      const u64 at = wr.at(i);
      fp[j] = i < n ? fps[at] : 0ull;
      const u32 lk = i < n ? keys[at] : 0u;
      slot[j] = (((u64)blockIdx.x * BS + (lk >> 8)) << 8) | (u64)(lk & 255u);
      // produced before by this workgroup's parents?  The first-come filter of orig_dedup_plain
      // (lds_first: a full probe window only lets a duplicate through to its owner's seen-set)
      if (fp[j] && !lds_first<ROUTE_FP_SLOTS>(lds_fp, fp[j])) fp[j] = 0;
      own[j] = fp[j] ? (int)fp_owner(fp[j], a.world) : -1;
      off[j] = own[j] >= 0 ? atomicAdd(&hist[own[j]], 1u) : 0u;
    }
    __syncthreads();
    if (threadIdx.x < a.world) base[threadIdx.x] = hist[threadIdx.x] ? atomicAdd(&a.rcnt_out[threadIdx.x], (unsigned long long)hist[threadIdx.x]) : 0ull;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < G; ++j) {
      if (own[j] < 0) continue;
      // one 16-B store per record
      *reinterpret_cast<ulonglong2*>(a.route + ((u64)own[j] * a.route_cap + base[own[j]] + off[j]) * 2) =
          make_ulonglong2((unsigned long long)fp[j], (unsigned long long)slot[j]);
    }
    __syncthreads();   // hist / base reused by the next round
  }
}

struct DedupShArgs {
  const u64* recv;             // (fp, slot) records of one source rank
  u64 n;
  u64* table;
  u64 table_mask;
  u64* reply;                  // compacted slots of the new ones
  unsigned long long* counter; // per-source reply count
  unsigned long long* ctr;
};

// owner-side insertion of one source rank's records into the seen-set as 8-B entries {fp} (no FIFO
// keys in sharded raft_original: twice the entries of the keyed table in the same bytes)
__global__ void __launch_bounds__(BS) orig_dedup_sh(DedupShArgs a) {
  __shared__ u32 wave_tot[BS / 64];
  __shared__ unsigned long long base_sh;
  const u64 tile = (u64)blockIdx.x * (BS * DEDUP_PER);
  u64 fp[DEDUP_PER], nk[DEDUP_PER], pos[DEDUP_PER];
#pragma unroll
  for (int j = 0; j < DEDUP_PER; ++j) {
    const u64 idx = tile + (u64)j * BS + threadIdx.x;
    fp[j] = idx < a.n ? a.recv[2 * idx] : 0ull;
    nk[j] = 0ull;
  }
  u32 err = 0;
  const u32 isnew = probe_batch<DEDUP_PER, false, 1>(a.table, a.table_mask, fp, nk, pos, err);
  u32 total = 0;
  const u32 off = block_excl_scan((u32)__popc(isnew), wave_tot, &total);
  if (threadIdx.x == 0) base_sh = total ? atomicAdd(a.counter, (unsigned long long)total) : 0ull;
  __syncthreads();
  u64 o = base_sh + off;
  for (int j = 0; j < DEDUP_PER; ++j) {
    if (!((isnew >> j) & 1u)) continue;
    const u64 idx = tile + (u64)j * BS + threadIdx.x;
    a.reply[o++] = a.recv[2 * idx + 1];
  }
  if (err) atomicOr(&a.ctr[K_ERR], (unsigned long long)err);
}

struct MatShArgs {
  const u32* states;
  const u64* acks;             // slots acknowledged as new by one owner
  u64 n, chunk_begin, chunk_count;
  u32* out;                    // [n][NWP + 4] state records for that owner
  u64 rank_bits;               // rank << 37
  u64 seed;
  OrigRuntime rt;
  unsigned long long* ctr;
  // the generator's own segment (it owns these states): straight into its store at st_dst
  // instead of a STATES record, when st_states is set
  u32* st_states;
  u64* st_meta;
  u64 st_dst, st_cap;
  u32 store;                   // 0: the last level of a depth-bounded search (count_final_level):
                               // counted and invariant-checked, neither stored nor shipped
};

template <class S>
__global__ void __launch_bounds__(BS) orig_materialize_sh(MatShArgs a) {
  using W = typename S::Work;
  constexpr int NW = S::NW, NWP = (S::NW + 3) & ~3, RW = NWP + 4;
  __shared__ unsigned int lds_cnt[OA_NACT];
  for (int t = threadIdx.x; t < OA_NACT; t += BS) lds_cnt[t] = 0;
  __syncthreads();
  const u64 i = (u64)blockIdx.x * BS + threadIdx.x;
  u32 err = 0;
  unsigned long long ev = ~0ull;
  if (i < a.n) {
    const u64 slot = a.acks[i];   // state in chunk << 8 | instance (orig_route_blk)
    const u64 k = slot & 255ull, gid = a.chunk_begin + (slot >> 8);
    u32 w[NWP];
    const uint4* src = reinterpret_cast<const uint4*>(a.states + gid * NWP);
#pragma unroll
    for (int q = 0; q < NWP / 4; ++q) { const uint4 v = src[q]; w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w; }
    W s, t;
    u64 al[S::AW];
    S::unpack(w, s);
    S::all_logs_next(s, al);
    u32 e2 = 0;
    const int act = S::apply(s, (int)k, t, e2);
#pragma unroll
    for (int q = 0; q < S::AW; ++q) t.allLogs[q] = al[q];
    u32 pw[NW];
    S::pack(t, pw);
    const u64 fp = fp64(pw, a.seed);
    const u64 meta = ((a.rank_bits | gid) << 24) | ((u64)(act < 0 ? 0 : act) << 16) | k;
    if (!a.store) {
      // counted only (count_final_level)
    } else if (a.st_states) {
      const u64 dst = a.st_dst + i;
      if (dst < a.st_cap) {
        uint4* o = reinterpret_cast<uint4*>(a.st_states + dst * NWP);
#pragma unroll
        for (int q = 0; q < NWP / 4; ++q)
          o[q] = make_uint4(pw[4 * q], 4 * q + 1 < NW ? pw[4 * q + 1] : 0u, 4 * q + 2 < NW ? pw[4 * q + 2] : 0u, 4 * q + 3 < NW ? pw[4 * q + 3] : 0u);
        a.st_meta[dst] = meta;
      } else {
        err |= OE_CAP_STORE;
      }
    } else {
      u32* o = a.out + i * RW;
#pragma unroll
      for (int q = 0; q < NWP / 4; ++q)
        reinterpret_cast<uint4*>(o)[q] = make_uint4(pw[4 * q], 4 * q + 1 < NW ? pw[4 * q + 1] : 0u, 4 * q + 2 < NW ? pw[4 * q + 2] : 0u, 4 * q + 3 < NW ? pw[4 * q + 3] : 0u);
      reinterpret_cast<uint4*>(o)[NWP / 4] = make_uint4((u32)meta, (u32)(meta >> 32), (u32)fp, (u32)(fp >> 32));
    }
    if (act >= 0) {
      atomicAdd(&lds_cnt[act], 1u);
      if (S::violated(t, a.rt.invariants & S::inv_frame(act))) ev = ev_word(gid, (u32)k, EV_VIOLATION);
    } else {
      err |= OE_TABLE_FULL;   // an acknowledged slot always re-derives
    }
  }
  if (err) atomicOr(&a.ctr[K_ERR], (unsigned long long)err);
  if (ev != ~0ull) atomicMin(&a.ctr[K_EVENT], ev);
  __syncthreads();
  for (int t = threadIdx.x; t < OA_NACT; t += BS)
    if (lds_cnt[t]) atomicAdd(&a.ctr[K_ACT + OA_NACT + t], (unsigned long long)lds_cnt[t]);
}

struct StoreArgs {
  const u32* in;               // [n][NWP + 4]
  u64 n, dst, cap;
  u32* states;
  u64* meta;
  unsigned long long* ctr;
};

template <int NWP>
__global__ void __launch_bounds__(BS) orig_store(StoreArgs a) {
  const u64 i = (u64)blockIdx.x * BS + threadIdx.x;
  if (i >= a.n) return;
  const u64 dst = a.dst + i;
  if (dst >= a.cap) { atomicOr(&a.ctr[K_ERR], (unsigned long long)OE_CAP_STORE); return; }
  const uint4* src = reinterpret_cast<const uint4*>(a.in + i * (NWP + 4));
  uint4* o = reinterpret_cast<uint4*>(a.states + dst * NWP);
#pragma unroll
  for (int q = 0; q < NWP / 4; ++q) o[q] = src[q];
  const uint4 m = src[NWP / 4];
  a.meta[dst] = (u64)m.x | ((u64)m.y << 32);
}

// Recovery from a checkpoint: re-insert the fingerprints of every stored state into the
// zeroed seen-set (the checkpoint holds states, not the table; FP64 is a function of the
// packed words, so the rebuilt set is the saved one).
template <class S, int STRIDE>
__global__ void __launch_bounds__(BS) orig_reinsert(const u32* states, u64 n, u64* table, u64 mask, u64 seed,
                                                    unsigned long long* ctr) {
  constexpr int NW = S::NW, NWP = (S::NW + 3) & ~3;
  const u64 i = (u64)blockIdx.x * BS + threadIdx.x;
  if (i >= n) return;
  u32 w[NW];
#pragma unroll
  for (int q = 0; q < NW; ++q) w[q] = states[i * NWP + q];
  // stored states are older than any successor the search will generate: key 0 (~key = ~0)
  const u64 fp[1] = {fp64(w, seed)}, nk[1] = {~0ull};
  u64 pos[1];
  u32 err = 0;
  probe_batch<1, STRIDE == 2, STRIDE>(table, mask, fp, nk, pos, err);
  if (err) atomicOr(&ctr[K_ERR], (unsigned long long)err);
}

#include "orig_sim.hip"   // simulation mode: the walker kernel and the host replay of one walk
#include "orig_sym.hip"   // SYMMETRY Permutations(Server): the orbit-fingerprint generate and reinsert kernels
#include "orig_reshard.hip"   // recovery at another GPU count: the classify / scan / place kernels

}  // namespace rmc
#include "dev_owner.h"   // host only, included here so that the device code above keeps its text
namespace rmc {

#define HIPCHK(x)                                                                             \
  do {                                                                                        \
    hipError_t e_ = (x);                                                                      \
    if (e_ != hipSuccess) { err = std::string(#x) + ": " + hipGetErrorString(e_); return MC_E_NO_DEVICE; } \
  } while (0)

template <class S>
class OrigGpu : public Backend {
 public:
  using W = typename S::Work;
  // S with the safety invariants (orig_spec.h §12) compiled into violated / inv_frame: what the host
  // evaluates, and the instantiation of every kernel that checks invariants when the cfg lists one
  // of them (safety()); a run that lists none launches the <S> kernels, whose code holds none of it
  using SS = WithSafety<S>;
  bool safety() const { return (m_.rt.invariants & OI_SAFETY_MASK) != 0; }
  // ... and with the action properties (orig_spec.h §14) as well: what the host evaluates a step with, and
  // (over S or SS) the instantiation of the generate and simulate kernels when the cfg lists PROPERTIES
  using SA = WithActions<SS>;
  bool actions() const { return m_.rt.action_props != 0; }
  static constexpr int NWP = (S::NW + 3) & ~3;
  explicit OrigGpu(const OrigModel& m) : m_(m) {}
  ~OrigGpu() override { release(); }

  std::string family() const override { return "raft_original"; }

  int observed_collision(double& v, std::string& err) override {
    if (!d_table_ || alloc_world_ != 0 || !run_table_) { err = "after a single-GPU mc_run only"; return MC_E_STATE; }
    // the table the run ended on: the starter, when the model never outgrew it
    return fpgap::observed(run_table_, run_mask_ + 1, last_fifo_ ? 2 : 1, stream_, v, err);
  }

  std::string describe_json() const override {
    std::ostringstream o;
    o << "{\"spec\": \"raft_original\", \"N\": " << S::N << ", \"NV\": " << S::NV << ", \"MaxTerm\": " << S::MT
      << ", \"MaxLogLen\": " << S::ML << ", \"MaxMsgDomain\": " << S::MK << ", \"MinMsgCount\": " << m_.rt.min_count
      << ", \"MaxMsgCount\": " << m_.rt.max_count << ", \"state_bits\": " << S::PBITS << ", \"state_words\": " << S::NW
      << ", \"state_bytes_stored\": " << NWP * 4 << ", \"instances\": " << S::NI << ", \"log_universe\": " << S::U
      << ", \"constraints\": [";
    for (size_t k = 0; k < m_.constraint_names.size(); ++k) o << (k ? ", " : "") << "\"" << m_.constraint_names[k] << "\"";
    o << "], \"invariants\": [";
    for (size_t k = 0; k < m_.inv_names.size(); ++k) o << (k ? ", " : "") << "\"" << m_.inv_names[k] << "\"";
    o << "], \"actions\": [";
    for (int k = 0; k < OA_NACT; ++k) o << (k ? ", " : "") << "\"" << kOrigActNames[k] << "\"";
    o << "]";
    // only under SYMMETRY (the description is also the checkpoint's model identity: a symmetric file
    // does not resume an unsymmetric search, nor the reverse, and unsymmetric files stay as they were)
    if (m_.rt.symmetry) o << ", \"symmetry\": true, \"permutations\": " << S::NPERM;
    // only with PROPERTIES, for the same reason: a checkpoint written with them does not resume without
    if (!m_.prop_names.empty()) {
      o << ", \"properties\": [";
      for (size_t k = 0; k < m_.prop_names.size(); ++k) o << (k ? ", " : "") << "\"" << m_.prop_names[k] << "\"";
      o << "]";
    }
    o << "}";
    return o.str();
  }

  // Buffers are allocated on the first run and reused (a re-run of the same
  // handle re-zeroes the seen-set and overwrites the store).
  int ensure_alloc(const RunOpts& o, int world, std::string& err) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= o.device) { err = "no HIP device available (raftmc has no CPU fallback)"; return MC_E_NO_DEVICE; }
    HIPCHK(hipSetDevice(o.device));
    if (d_table_ && o.device == dev_ && o.fp_table_bytes == req_table_ && o.state_store_bytes == req_store_ && world == alloc_world_) return 0;
    release();
    size_t freeb = 0, totalb = 0;
    HIPCHK(hipMemGetInfo(&freeb, &totalb));
    uint64_t tb = o.fp_table_bytes ? o.fp_table_bytes : std::min<uint64_t>(8ull << 30, freeb / 4);
    uint64_t slots = 1; while (slots * 2 * 16 <= tb) slots *= 2;   // 16-B entries {fp, ~key}
    if (slots < 1024) slots = 1024;
    uint64_t sb = o.state_store_bytes ? o.state_store_bytes : std::min<uint64_t>(32ull << 30, freeb / 3);
    const u64 cap = std::max<u64>(16, sb / (NWP * 4 + 8));
    // frontier chunk: the record regions hold chunk_states * NI records (10 B each), their
    // distinct pairs (16 B) and the inserted-position list as many 8-B entries (worst case: every
    // record new), sharded mode also world route regions of 16-B records: ~1/4 of the store
    chunk_states_ = std::max<u64>(4096, std::min<u64>(cap, (sb / 4) / ((34 + 16 * (u64)world) * (u64)S::NI)));
    chunk_states_ = std::min<u64>(chunk_states_, (u64)SCAN_BS * 64 * BS);   // orig_scan: <= 64 blocks per lane
    chunk_states_ = (chunk_states_ / BS) * BS;   // whole workgroups: records are grouped per generate workgroup
    const u64 nblk = chunk_states_ / BS, nrec = chunk_states_ * (u64)S::NI;
    table_mask_ = slots - 1;
    HIPCHK(res_.device(&d_table_, slots * 16));
    HIPCHK(store_.alloc(cap, NWP));
    HIPCHK(res_.device(&d_rfp_, nrec * 8));
    HIPCHK(res_.device(&d_rkey_, nrec * 2));
    HIPCHK(res_.device(&d_rcnt_blk_, nblk * 16));
    HIPCHK(res_.device(&d_newrec_, nrec * 8));          // inserted entry positions (single GPU) / replies (sharded)
    HIPCHK(res_.device(&d_urec_, nrec * 16));           // distinct (fp, ~key) per workgroup region
    HIPCHK(res_.device(&d_ucnt_, nblk * 4));
    HIPCHK(res_.device(&d_winmask_, chunk_states_ * WW * 8));
    HIPCHK(res_.device(&d_wcnt_, nblk * 4));
    HIPCHK(res_.device(&d_woff_, nblk * 8));
    HIPCHK(res_.device(&d_lead_, chunk_states_ * 4));
    HIPCHK(res_.device(&d_ctr_, K_NCTR * 8));
    HIPCHK(res_.pinned(&h_ctr_, K_NCTR * 8));
    HIPCHK(res_.device(&d_stop_, (1 + OA_NACT) * 8));
    HIPCHK(hipMemset(d_winmask_, 0, chunk_states_ * WW * 8));
    if (world >= 1) {   // sharded mode
      HIPCHK(res_.device(&d_route_, (u64)world * nrec * 16));
      HIPCHK(res_.device(&d_rcnt_, 2 * 8 * 8));
    }
    HIPCHK(res_.stream(&stream_, hipStreamNonBlocking));
    HIPCHK(res_.event(&ctr_ev_, hipEventDisableTiming));
    if (world == 0) {   // single-GPU run(): the full table's clear runs on a stream of its own beside the first levels
      HIPCHK(res_.stream(&clear_stream_, hipStreamNonBlocking));
      HIPCHK(res_.event(&clear_ev_, hipEventDisableTiming));
      HIPCHK(res_.event(&gen_ev_, hipEventDisableTiming));
      // the level hoist (launch_hoist): the hoisted pair's counters, the stream and the events of the
      // host's look at K_LEVEL_NEW, and the pair's timing events (two pairs: a level reads its own
      // after the next hoist has been queued)
      HIPCHK(res_.device(&d_ctr2_, K_NCTR * 8));
      HIPCHK(res_.pinned(&h_x_, 8));
      HIPCHK(res_.stream(&x_stream_, hipStreamNonBlocking));
      HIPCHK(res_.event(&x_ev_, hipEventDisableTiming));
      HIPCHK(res_.event(&hx_ev_, hipEventDisableTiming));
      for (int i = 0; i < 4; ++i) HIPCHK(res_.event(&hoist_ev_[i / 2][i % 2]));
      if (2 * slots >= STARTER_FACTOR * STARTER_SLOTS)
        if (int rc = ensure_starter(STARTER_SLOTS, err)) return rc;
    }
    dev_ = o.device; req_table_ = o.fp_table_bytes; req_store_ = o.state_store_bytes; alloc_world_ = world;
    return 0;
  }

  // The starter seen-set: a small table the search begins on while the full table's clear (pure
  // bandwidth, 1.4 ms for 4 GiB) runs on clear_stream_ beside the first levels (pure launch
  // latency).  STARTER_SLOTS entries of the run's layout (8 B, or 16 B in FIFO order), used when
  // the full table has at least STARTER_FACTOR times as many; RAFTMC_STARTER_SLOTS (read per run):
  // 0 = no starter, a power of two = that many slots whatever the full table's size.
  // 2^23 slots (profiles/r07_overlap_ab.txt): C2 leaves it after 8 levels, when the
  // 4 GiB clear has just ended, and its own clear and orig_migrate's walk (64 MiB each) are the
  // cheapest; 2^24 and 2^25 stay one level longer, 2^26 two, and pay 2x to 8x for both.
  static constexpr u64 STARTER_SLOTS = 1ull << 23, STARTER_FACTOR = 8;
  int ensure_starter(u64 slots, std::string& err) {
    if (d_starter_ && starter_cap_ == slots) return 0;
    if (d_starter_) HIPCHK(hipStreamSynchronize(stream_));
    starter_cap_ = 0;
    HIPCHK(res_.device(&d_starter_, slots * 16));   // (frees the old one first)
    starter_cap_ = slots;
    return 0;
  }

  // timing events come from one pool that grows on demand (DevOwner::pool_event); null: the runtime refused one
  hipEvent_t pool_ev(size_t i) { return (hipEvent_t)res_.pool_event(i); }

  // rec0: the chunk's record buffers start this many parents into the allocations (run()'s pipelined
  // levels alternate between the two halves, chunk_plan.h; a multiple of BS)
  GenArgs gen_args(u64 dev_begin, u64 count, u64 gid0, u64 seed, const RunOpts& o, u64 rec0 = 0) const {
    GenArgs g;
    g.states = store_.states(); g.chunk_begin = dev_begin; g.chunk_count = count; g.gid0 = gid0;
    g.rfp = d_rfp_ + rec0 * S::NI; g.rkey = d_rkey_ + rec0 * S::NI; g.rcnt = d_rcnt_blk_ + rec0 / BS * 4; g.seed = seed; g.rt = m_.rt;
    g.inv_oom = o.inv_out_of_model ? 1u : 0u; g.deadlock = o.check_deadlock ? 1u : 0u;
    g.ctr = (unsigned long long*)d_ctr_;
    g.lead = d_lead_ + rec0;
    return g;
  }

  // the successor pass of one chunk: orig_generate over every parent, then orig_generate_lead over
  // the parents with leader work (its grid strides over the count the first kernel left on the
  // device); K_LEAD must be zero before (level start: orig_reset_ctr, later chunks: orig_advance, or
  // on a pipelined level the generate stream's own re-arm)
  void launch_generate(const GenArgs& g, unsigned nblk, hipStream_t st) {
    if (actions()) {
      if (safety()) launch_generate_as<WithActions<SS>>(g, nblk, st);
      else launch_generate_as<WithActions<S>>(g, nblk, st);
    } else if (safety()) launch_generate_as<SS>(g, nblk, st);
    else launch_generate_as<S>(g, nblk, st);
  }
  template <class K>   // K: S or SS, or WithActions of either
  void launch_generate_as(const GenArgs& g, unsigned nblk, hipStream_t st) {
    if (m_.rt.symmetry) {   // orbit fingerprints, every instance in one kernel (orig_sym.hip)
      hipLaunchKernelGGL((orig_generate_sym<K>), dim3(nblk), dim3(BS), 0, st, g);
      return;
    }
    hipLaunchKernelGGL((orig_generate<K>), dim3(nblk), dim3(BS), 0, st, g);
    const unsigned lblk = std::min<unsigned>(nblk, std::max<unsigned>(64u, nblk / 8));
    hipLaunchKernelGGL((orig_generate_lead<K>), dim3(lblk), dim3(BS), 0, st, g);
  }

  RouteArgs route_args(u32 world) const {
    RouteArgs ra;
    ra.rfp = d_rfp_; ra.rkey = d_rkey_; ra.rcnt = d_rcnt_blk_; ra.region = (u64)BS * S::NI; ra.route = d_route_;
    ra.route_cap = chunk_states_ * S::NI; ra.world = world; ra.rcnt_out = (unsigned long long*)d_rcnt_;
    return ra;
  }

  // the seen-set pass over the records g's generate left, against the table the search is on (run()
  // may be on the starter): orig_merge + orig_probe in FIFO order, orig_dedup_plain otherwise
  DedupArgs dedup_args(const GenArgs& g, u64 gid0, u64* tbl, u64 tmask) const {
    DedupArgs d;
    d.rfp = g.rfp; d.rkey = g.rkey; d.rcnt = g.rcnt; d.region = (u64)BS * S::NI; d.gid0 = gid0;
    d.urec = (ulonglong2*)d_urec_; d.ucnt = d_ucnt_;
    d.table = tbl; d.table_mask = tmask; d.newpos = d_newrec_; d.ctr = (unsigned long long*)d_ctr_;
    d.prof = prof_ ? 1u : 0u;
    return d;
  }
  // beside_generate: the instantiation that shares a CU with orig_generate.  The
  // dispatcher gives freed wave slots to whatever fits first, and a dedup workgroup fits long before a
  // generate workgroup (4 x 128 VGPRs): 8 per CU take the whole device and generate advances at a fifth of
  // its speed until the probes end.  The 4096-slot filter holds a CU to 4 (the best of 3 to 6 at either
  // batch size), and at 2 probes per thread (4 x 32 VGPRs) three generate waves per SIMD fit beside them
  void launch_dedup_plain(const DedupArgs& d, unsigned nblk, bool beside_generate, bool count_probes) {
    if (beside_generate) {
      if (count_probes) hipLaunchKernelGGL((orig_dedup_plain<WW, true, OVERLAP_DEDUP_PER, OVERLAP_LDS_FP_SLOTS, true>), dim3(nblk), dim3(BS), OVERLAP_FILTER_LDS, stream_, d);
      else hipLaunchKernelGGL((orig_dedup_plain<WW, false, OVERLAP_DEDUP_PER, OVERLAP_LDS_FP_SLOTS, true>), dim3(nblk), dim3(BS), OVERLAP_FILTER_LDS, stream_, d);
    } else {
      if (count_probes) hipLaunchKernelGGL((orig_dedup_plain<WW, true>), dim3(nblk), dim3(BS), 0, stream_, d);
      else hipLaunchKernelGGL((orig_dedup_plain<WW, false>), dim3(nblk), dim3(BS), 0, stream_, d);
    }
  }

  // the -workers N store pass: the new states of a chunk of cnt parents, from the positions
  // orig_dedup_plain left in d_newrec_, behind dst_base (a device slot); store = false: counted
  // and checked only (count_final_level).  base: global id of device slot 0
  MatPlainArgs mat_plain_args(u64 base, u64 dst_base, bool store) const {
    MatPlainArgs m;
    m.states = store_.states(); m.meta = store_.meta(); m.newrec = d_newrec_; m.base = base; m.dst_base = dst_base;
    m.cap = store_.cap(); m.rt = m_.rt; m.ctr = (unsigned long long*)d_ctr_; m.store = store ? 1u : 0u;
    return m;
  }
  void launch_materialize_plain(const MatPlainArgs& m, u64 cnt) {
    const dim3 grid((unsigned)std::min<u64>(4096, (cnt * 2 + BS - 1) / BS));
    if (safety()) hipLaunchKernelGGL((orig_materialize_plain<SS>), grid, dim3(BS), 0, stream_, m);
    else hipLaunchKernelGGL((orig_materialize_plain<S>), grid, dim3(BS), 0, stream_, m);
  }

  // ---------------------------------------------------------------- sharded stages
  // What the step API (shard_generate .. shard_store, driven by shard.py) and the native level loop
  // (shard_run_native) both queue on stream_; neither stage waits for the device.  Each kernel
  // launch sits in an event pair of its own (timed), read back by harvest() at the caller's next
  // host synchronisation.
  struct Seg { const u64* p; u64 n; };   // one rank's segment of an exchange: records, how many

  template <class F>
  int timed(int k, F&& launch, std::string& err) {
    const size_t i = pending_.size();
    hipEvent_t const e0 = pool_ev(2 * i), e1 = pool_ev(2 * i + 1);
    if (!e0 || !e1) { err = "hipEventCreate failed"; return MC_E_NO_DEVICE; }
    HIPCHK(hipEventRecord(e0, stream_));
    launch();
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e1, stream_));
    pending_.push_back(k);
    sres_.kernels[k].launches++;
    return 0;
  }
  void harvest() {
    for (size_t i = 0; i < pending_.size(); ++i) {
      float ms = 0;
      (void)hipEventElapsedTime(&ms, pool_ev(2 * i), pool_ev(2 * i + 1));
      sres_.kernels[pending_[i]].ms += ms;
    }
    pending_.clear();
  }

  // grow-only device buffer of cap bytes (what it held is not kept)
  template <class T>
  int grow(T*& p, u64& cap, u64 need, std::string& err) {
    if (need <= cap) return 0;
    if (p) { HIPCHK(hipStreamSynchronize(stream_)); res_.free(&p); }
    cap = 0;
    const u64 want = std::max<u64>(need + need / 4, 1 << 20);
    HIPCHK(res_.device(&p, want));
    cap = want;
    return 0;
  }

  // the chunk sh_chunk_begin_ / sh_chunk_count_ (not empty) of this rank's frontier
  GenArgs sh_gen_args() const { return gen_args(sh_chunk_begin_, sh_chunk_count_, sh_chunk_begin_, sres_.seed, sopts_); }
  int stage_generate(const GenArgs& g, unsigned nblk, std::string& err) {
    HIPCHK(hipMemsetAsync(d_ctr_ + K_LEAD, 0, 8, stream_));
    if (int rc = timed(0, [&] { launch_generate(g, nblk, stream_); }, err)) return rc;
    sres_.kernels[0].algo_bytes += (double)sh_chunk_count_ * NWP * 4;
    return 0;
  }

  // generate + route of that chunk: the successors' (fp, slot) records bucketed by owner into
  // d_route_, the per-owner counts in d_rcnt_[0, 8)
  int stage_generate_route(std::string& err) {
    HIPCHK(hipMemsetAsync(d_rcnt_, 0, 8 * 8, stream_));
    if (!sh_chunk_count_) return 0;
    const unsigned nblk = (unsigned)((sh_chunk_count_ + BS - 1) / BS);
    if (int rc = stage_generate(sh_gen_args(), nblk, err)) return rc;
    const RouteArgs ra = route_args((u32)world_);
    return timed(1, [&] { hipLaunchKernelGGL(orig_route_blk, dim3(nblk), dim3(BS), 0, stream_, ra); }, err);
  }

  // owner side: the records received from each source rank (seg[r]; at most one chunk's worth in
  // all) against this rank's seen-set, one launch per non-empty segment; the new ones' slots are
  // packed at d_newrec_ + seg_off_[r], their counts in d_rcnt_[8, 16)
  int stage_dedup(const Seg* seg, std::string& err) {
    HIPCHK(hipMemsetAsync(d_rcnt_ + 8, 0, 8 * 8, stream_));
    u64 off = 0;
    for (int r = 0; r < world_; ++r) {
      seg_off_[r] = off;
      const u64 n = seg[r].n;
      if (n) {
        DedupShArgs d;
        d.recv = seg[r].p; d.n = n; d.table = d_table_; d.table_mask = sh_table_mask();
        d.reply = d_newrec_ + off; d.counter = (unsigned long long*)(d_rcnt_ + 8 + r); d.ctr = (unsigned long long*)d_ctr_;
        if (int rc = timed(2, [&] { hipLaunchKernelGGL(orig_dedup_sh, dim3((unsigned)((n + BS * DEDUP_PER - 1) / (BS * DEDUP_PER))), dim3(BS), 0, stream_, d); }, err))
          return rc;
      }
      off += n;
    }
    return 0;
  }

  // generator side: the acknowledged slots of the current chunk (ack[r]: from owner r) become
  // states again, invariant-checked and counted per action; packed with their parent pointers at
  // d_stout_ + seg_off_ack_[r] records for the STATES exchange.  own >= 0: segment `own` is this
  // rank's, and its states also go straight into the store at own_dst.  last: a counted final
  // level, nothing is written
  int stage_rederive(const Seg* ack, bool last, int own, u64 own_dst, std::string& err) {
    const u64 SBW = (u64)(NWP + 4) * 4;   // STATES record bytes
    u64 total = 0;
    for (int r = 0; r < world_; ++r) { seg_off_ack_[r] = total; total += ack[r].n; }
    if (!last)
      if (int rc = grow(d_stout_, stout_cap_, total * SBW, err)) return rc;
    for (int r = 0; r < world_; ++r) {
      if (!ack[r].n) continue;
      MatShArgs m;
      m.states = store_.states(); m.acks = ack[r].p; m.n = ack[r].n; m.chunk_begin = sh_chunk_begin_;
      m.chunk_count = sh_chunk_count_; m.out = last ? nullptr : d_stout_ + seg_off_ack_[r] * (NWP + 4); m.rank_bits = (u64)rank_ << 37;
      m.seed = sres_.seed; m.rt = m_.rt; m.ctr = (unsigned long long*)d_ctr_;
      m.st_states = nullptr; m.st_meta = nullptr; m.st_dst = 0; m.st_cap = 0; m.store = last ? 0u : 1u;
      if (r == own && !last) { m.st_states = store_.states(); m.st_meta = store_.meta(); m.st_dst = own_dst; m.st_cap = store_.cap(); }
      const dim3 grid((unsigned)((m.n + BS - 1) / BS));
      if (int rc = timed(3, [&] {
            if (safety()) hipLaunchKernelGGL((orig_materialize_sh<SS>), grid, dim3(BS), 0, stream_, m);
            else hipLaunchKernelGGL((orig_materialize_sh<S>), grid, dim3(BS), 0, stream_, m);
          }, err))
        return rc;
    }
    sres_.kernels[3].algo_bytes += (double)total * (8 + NWP * 4 + (last ? 0 : SBW));
    return 0;
  }

  // owner side: n received STATES records into the store behind what the level has stored so far
  int stage_store(const u32* in, u64 n, std::string& err) {
    StoreArgs a;
    a.in = in; a.n = n; a.dst = sh_next_write_; a.cap = store_.cap(); a.states = store_.states(); a.meta = store_.meta();
    a.ctr = (unsigned long long*)d_ctr_;
    if (int rc = timed(4, [&] { hipLaunchKernelGGL((orig_store<NWP>), dim3((unsigned)((n + BS - 1) / BS)), dim3(BS), 0, stream_, a); }, err))
      return rc;
    sres_.kernels[4].algo_bytes += (double)n * ((NWP + 4) * 4 + NWP * 4 + 8);
    sh_next_write_ += n; sh_new_ += n;
    return 0;
  }

  // an empty result of this model: the fingerprint seed and the per-kernel entries of the caller's pipeline
  static u64 bfs_seed(const RunOpts& o) { return o.seed ? o.seed : 0x5EED5EED2024ull; }
  static RunResult new_result(u64 seed, std::initializer_list<const char*> kernels) {
    RunResult r;
    r.seed = seed;
    r.state_bytes = NWP * 4;
    for (int k = 0; k < OA_NACT; ++k) r.action_names.push_back(kOrigActNames[k]);
    r.act_generated.assign(OA_NACT, 0); r.act_distinct.assign(OA_NACT, 0);
    for (const char* k : kernels) r.kernels.push_back({k, 0, 0, 0});
    return r;
  }

  // ---------------------------------------------------------------- simulation mode (orig_sim.hip)
  bool supports_simulation() const override { return true; }

  static u32 sim_depth(const RunOpts& o) { return (u32)(o.max_depth > 0 ? o.max_depth : SIM_DEFAULT_DEPTH); }
  static int sim_check(const RunOpts& o, std::string& err) {
    if (o.max_depth > SIM_MAX_DEPTH) { err = "simulation: depth is at most " + std::to_string(SIM_MAX_DEPTH); return MC_E_INVALID; }
    if (o.sim_walks > SIM_MAX_WALKS) { err = "simulation: at most 2^40 walks"; return MC_E_INVALID; }
    if (o.sim_batch < 0 || o.sim_batch > (1ll << 30)) { err = "simulation: batch out of range"; return MC_E_INVALID; }
    return 0;
  }

  int sim_walk(const RunOpts& o, int64_t walk, std::string& text, std::string& err) override {
    if (int rc = sim_check(o, err)) return rc;
    if (walk < 0 || walk >= SIM_MAX_WALKS) { err = "simulation: walk number out of range"; return MC_E_INVALID; }
    SimWalk<SA> w;
    sim_replay<SA>(m_.rt, o.inv_out_of_model, o.check_deadlock, o.seed, (u64)walk, sim_depth(o), w);
    text.clear();
    for (const W& st : w.states) { text += state_text(st, false); text += "\n"; }
    return 0;
  }

  // RunOpts::sim_walks random walks in batches of sim_batch walkers, one orig_simulate launch per
  // batch; the run stops after the first batch that records an event.  Allocates the counters only:
  // no seen-set, no store (the BFS buffers of an earlier run() of this handle are left alone).
  int simulate(const RunOpts& o, RunResult& r, std::string& err) {
    if (int rc = sim_check(o, err)) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= o.device) { err = "no HIP device available (raftmc has no CPU fallback)"; return MC_E_NO_DEVICE; }
    HIPCHK(hipSetDevice(o.device));
    const auto t0 = std::chrono::steady_clock::now();
    const u32 depth = sim_depth(o);
    const u64 num = (u64)o.sim_walks, batch = (u64)(o.sim_batch ? o.sim_batch : SIM_DEFAULT_BATCH);
    r = new_result(o.seed, {"orig_simulate"});   // (the walks' seed is the caller's, 0 included)
    r.simulated = true;
    W s0; S::init(s0);
    r.depth = 1;   // generated: the successors evaluated along the walks (Init is not counted)
    if (!S::in_model(s0, m_.rt)) { err = "the initial state violates a state constraint"; r.verdict = MC_VERDICT_OK; return 0; }
    if (u32 bad = SS::violated(s0, m_.rt.invariants)) {
      r.verdict = MC_VERDICT_INVARIANT_VIOLATION; r.violated = first_violated(bad);
      r.trace.push_back({"<Initial predicate>", state_text(s0, true)});
      r.seconds_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      return 0;
    }
    // device counters, freed on every way out
    struct Dev { unsigned long long* ctr = nullptr; hipEvent_t e0 = nullptr, e1 = nullptr; DevOwner<HipDevApi> own; } d;
    HIPCHK(d.own.device(&d.ctr, SK_NCTR * 8));
    HIPCHK(d.own.event(&d.e0));
    HIPCHK(d.own.event(&d.e1));
    u64 h[SK_NCTR], event = ~0ull, maxlen = 1;
    for (u64 w0 = 0; w0 < num && event == ~0ull; w0 += batch) {
      const u64 n = std::min<u64>(batch, num - w0);
      std::memset(h, 0, sizeof h);
      h[SK_EVENT] = ~0ull;
      HIPCHK(hipMemcpy(d.ctr, h, sizeof h, hipMemcpyHostToDevice));
      SimArgs a;
      a.walk0 = w0; a.nwalks = n; a.seed = o.seed; a.depth = depth; a.rt = m_.rt;
      a.inv_oom = o.inv_out_of_model ? 1u : 0u; a.deadlock = o.check_deadlock ? 1u : 0u; a.ctr = d.ctr;
      HIPCHK(hipEventRecord(d.e0, nullptr));
      const dim3 grid((unsigned)((n + BS - 1) / BS));
      if (actions()) {
        if (safety()) hipLaunchKernelGGL((orig_simulate<WithActions<SS>>), grid, dim3(BS), 0, nullptr, a);
        else hipLaunchKernelGGL((orig_simulate<WithActions<S>>), grid, dim3(BS), 0, nullptr, a);
      } else if (safety()) hipLaunchKernelGGL((orig_simulate<SS>), grid, dim3(BS), 0, nullptr, a);
      else hipLaunchKernelGGL((orig_simulate<S>), grid, dim3(BS), 0, nullptr, a);
      HIPCHK(hipGetLastError());
      HIPCHK(hipEventRecord(d.e1, nullptr));
      HIPCHK(hipMemcpy(h, d.ctr, sizeof h, hipMemcpyDeviceToHost));
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, d.e0, d.e1));
      r.kernels[0].ms += ms; r.kernels[0].launches += 1; r.n_launches += 1;
      r.seconds_kernels += ms * 1e-3;
      r.sim_walks_run += (int64_t)n;
      r.sim_steps += (int64_t)h[SK_STEPS];
      for (int k = 0; k < OA_NACT; ++k) { r.act_generated[k] += (int64_t)h[SK_ACT + k]; r.generated += (int64_t)h[SK_ACT + k]; }
      maxlen = std::max<u64>(maxlen, h[SK_MAXLEN]);
      if (progress_)
        std::fprintf(stderr, "simulation: walks %llu..%llu, %llu steps, %.3f ms\n", (unsigned long long)w0,
                     (unsigned long long)(w0 + n - 1), (unsigned long long)h[SK_STEPS], ms);
      if (h[SK_ERR]) {
        r.verdict = MC_VERDICT_CAPACITY_OVERFLOW;
        r.error = (h[SK_ERR] & OE_CAP_ELECTIONS) ? "elections set exceeds the compiled capacity" : "message count outside the packed range";
        r.depth = (int64_t)maxlen;
        r.seconds_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return 0;
      }
      event = h[SK_EVENT];
    }
    r.depth = (int64_t)maxlen;
    if (event != ~0ull) {
      // the winning walk again, on the host, with the same spec code and draws
      const u64 walk = sim_event_walk(event);
      SimWalk<SA> w;
      sim_replay<SA>(m_.rt, o.inv_out_of_model, o.check_deadlock, o.seed, walk, depth, w);
      if (w.event != event) {
        err = "simulation: the host replay of walk " + std::to_string(walk) + " does not reproduce the device's event";
        return MC_E_STATE;
      }
      r.sim_event_walk = (int64_t)walk;
      const u32 kind = sim_event_kind(event);
      if (kind == EV_VIOLATION) {
        name_violation(w.states[w.states.size() - 2], w.states.back(), (int)sim_event_inst(event), o.inv_out_of_model, r.verdict, r.violated);
      } else if (kind == EV_DEADLOCK) {
        r.verdict = MC_VERDICT_DEADLOCK;
      } else {
        r.verdict = MC_VERDICT_EVAL_ERROR;
        r.error = "TLC evaluation error while computing the successors of the last state of walk " + std::to_string(walk) +
                  ": log[i][prevLogIndex] applied outside its domain (raft_original.tla:207-210)";
      }
      for (size_t k = 0; k < w.states.size(); ++k)
        r.trace.push_back({k == 0 ? std::string("<Initial predicate>") : std::string(kOrigActNames[w.acts[k - 1]]), state_text(w.states[k], true)});
    } else {
      r.verdict = MC_VERDICT_OK;
    }
    r.seconds_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return 0;
  }

  // ================================================================ the single-GPU search
  // One run's state, shared by run()'s level loop and its stages below.
  struct Search {
    std::chrono::steady_clock::time_point t0;
    bool fifo = false;           // TLC -workers 1: single-worker FIFO order (16-B {fp, ~key} entries); -workers N: 8-B entries
    bool count_probes = false;   // count the seen-set probes of the -workers N pipeline (an instrumented kernel)
    bool count_last = false;     // count_final_level applies to this run
    u64* tbl = nullptr;          // the table the search is on, and its entry mask
    u64 tmask = 0, full_mask = 0, st_slots = 0;   // st_slots: the starter's (0: begun on the full table)
    u64 level_begin = 0, level_count = 1;
    ChunkPlan plan{0, 0, 0};
    // the level being expanded: counted not stored, pipelined, its chunks, and what read_level found
    bool last = false, ovl = false;
    int nch = 0;
    u64 nnew = 0;
    double level_ms = 0;
    // the level hoist (launch_hoist): a level's first `count` parents generated ahead, beside the level
    // before's last dedup, into half `buffer`, timed by hoist_ev_[slot].  cur: this level's chunk 0;
    // next: queued for the level after this one (what drain_hoist gives up).  arm: this level's last
    // dedup leaves room for one
    struct Hoist { u64 count = 0; int buffer = 0, slot = 0; };
    Hoist cur, next;
    bool hoist_on = false, arm = false;
    u64 hoist_min = 0;
    u64 level_end() const { return level_begin + level_count; }
  };

  // Set up, then per level: spill?, switch to the full table?, queue the level's kernels, read its
  // counters back (the level's one host wait), decide.
  int run(const RunOpts& o, RunResult& r, std::string& err) override {
    if (o.sim_walks > 0) return simulate(o, r, err);   // TLC -simulate: random walks, not a BFS (no fingerprints: SYMMETRY is ignored)
    if (m_.rt.symmetry && o.count_final_level) { err = "SYMMETRY for raft_original: not with count_final_level"; return MC_E_UNSUPPORTED; }
    unstored_ = 0;   // a previous run's unstored level must not outlive it (mc_dump_states)
    if (int rc = ensure_alloc(o, 0, err)) return rc;   // world 0 = single-GPU pipeline
    Search s;
    s.t0 = std::chrono::steady_clock::now();
    s.fifo = o.workers == 1;
    last_fifo_ = s.fifo;
    // RAFTMC_COUNT_PROBES: read per run, so a caller can count in a run of its own outside a timed region
    s.count_probes = std::getenv("RAFTMC_COUNT_PROBES") != nullptr;
    if (int rc = begin_search(o, s, err)) return rc;
    r = new_result(bfs_seed(o), {"orig_generate", "orig_merge_probe", "orig_mark_scan", "orig_materialize"});
    store_.reset();
    bool ended = false;
    if (int rc = init_level0(o, s, r, ended, err)) return rc;
    if (ended) return 0;
    // count_final_level: the level at depth max_depth is never expanded, so the -workers N search
    // counts and checks its states without storing them (an event re-runs FIFO, which stores all)
    s.count_last = o.count_final_level && !s.fifo && o.max_depth > 0 && o.checkpoint_path.empty();
    unstored_ = 0;
    // RAFTMC_OVERLAP_STATES (read per run): the sub-chunk size of a pipelined level; 0 = every level
    // on one stream, any other value a forced size (whole workgroups) that pipelines every level
    // with more parents than one sub-chunk.  RAFTMC_OVERLAP_MIN_LEVEL: the smallest pipelined level.
    const u64 sub_env = env_u64("RAFTMC_OVERLAP_STATES", ~0ull);
    // (the FIFO path is never split)
    s.plan = ChunkPlan(chunk_states_, s.fifo ? 0 : sub_env == ~0ull ? ChunkPlan::default_sub(chunk_states_) : sub_env,
                       env_u64("RAFTMC_OVERLAP_MIN_LEVEL", sub_env == ~0ull ? OVERLAP_MIN_LEVEL : 0), BS);
    // RAFTMC_HOIST (read per run): 0 = no level hoist (launch_hoist); RAFTMC_HOIST_MIN: the fewest
    // parents worth generating ahead
    s.hoist_on = !s.fifo && env_u64("RAFTMC_HOIST", 1) != 0;
    s.hoist_min = std::max<u64>(BS, env_u64("RAFTMC_HOIST_MIN", OVERLAP_MIN_HALF));
    const u64 S_B = NWP * 4;
    // an exit from the loop gives up a queued hoist first (drain_hoist)
    auto leave = [&](int rc) { std::string e2; (void)drain_hoist(s, e2); return rc; };
    while (s.level_count > 0) {
      if (o.max_depth && r.depth >= o.max_depth) {
        if (int rc = drain_hoist(s, err)) return rc;
        r.left_on_queue = (int64_t)s.level_count; r.verdict = MC_VERDICT_DEPTH_LIMIT; break;
      }
      s.last = s.count_last && r.depth + 1 >= o.max_depth;
      if (int rc = maybe_spill(s, r, err)) return leave(rc);
      if (!ctr_clean_) {
        hipLaunchKernelGGL(orig_reset_ctr, dim3(1), dim3(64), 0, stream_, (unsigned long long*)d_ctr_);
        HIPCHK(hipGetLastError());
      }
      ctr_clean_ = false;
      if (int rc = maybe_switch_to_full_table(s, r, err)) return leave(rc);
      s.cur = s.next; s.next = typename Search::Hoist();
      if (int rc = fold_hoist(s, err)) return rc;
      // a split level generates the next level's first parents beside its last dedup when that level
      // will be expanded (this one is not the counted last, max_depth does not stop it) and no
      // checkpoint is written between the two
      s.arm = s.hoist_on && !s.last && (s.cur.count || s.plan.split(s.level_count)) &&
              !(o.max_depth && r.depth + 1 >= o.max_depth) &&
              !(o.checkpoint_every > 0 && !o.checkpoint_path.empty() && (r.depth + 1) % o.checkpoint_every == 0);
      if (int rc = queue_level(o, s, r, err)) return leave(rc);
      if (s.arm)
        if (int rc = launch_hoist(o, s, r, err)) return leave(rc);
      if (int rc = read_level(s, r, err)) return leave(rc);
      u64* const c = h_ctr_;
      const u64 level_end = s.level_end(), nnew = s.nnew;
      if (!s.last && level_end + nnew - store_.base() > store_.cap()) c[K_ERR] |= OE_CAP_STORE;
      const bool event = c[K_EVENT] != ~0ull && (c[K_ERR] & ~(u64)OE_CAP_STORE) == 0;
      // the search stops or starts over here, or the next level is not what the hoist took it for
      if (event || c[K_ERR] || s.next.count > nnew)
        if (int rc = drain_hoist(s, err)) return rc;
      if (event && !s.fifo) return research_fifo(o, c[K_EVENT], r, err);
      if (event) {
        // the level's first event in TLC's order stops the search; a full state store only
        // matters when it cut off states that come before the event in key order
        const u64 stored = std::min<u64>(nnew, store_.cap() - std::min<u64>(store_.cap(), level_end - store_.base()));
        bool decided = false;
        if (int rc = handle_event(c[K_EVENT], s.level_begin, s.level_count, nnew, stored, o.inv_out_of_model, r, decided, err)) return rc;
        if (decided) { store_.set_total(level_end + stored); break; }
      }
      if (c[K_ERR]) {
        r.verdict = MC_VERDICT_CAPACITY_OVERFLOW;
        r.error = capacity_error(c, level_end, nnew, r.depth);
        store_.set_total(level_end);
        r.distinct = (int64_t)level_end;
        break;
      }
      int64_t gen = 0;
      for (int k = 0; k < OA_NACT; ++k) { r.act_generated[k] += (int64_t)c[K_ACT + k]; r.act_distinct[k] += (int64_t)c[K_ACT + OA_NACT + k]; gen += (int64_t)c[K_ACT + k]; }
      r.generated += gen;
      r.generated_in_model += (int64_t)c[K_GEN_IN];
      r.seen_set_probes += (int64_t)c[K_PROBES];
      r.algo_bytes += (double)s.level_count * S_B + (double)c[K_GEN_IN] * 8 + (double)nnew * (16 + S_B);
      if (s.last) unstored_ = nnew;   // counted, not in the store (the store's total counts stored states)
      else store_.set_total(store_.total() + nnew);
      r.distinct = (int64_t)(store_.total() + unstored_);
      r.levels.back().generated = gen;
      r.levels.back().kernel_ms = s.level_ms;
      if (nnew > 0) { r.levels.push_back({(int64_t)nnew, 0, 0.0}); r.depth += 1; }
      s.level_begin += s.level_count;
      s.level_count = nnew;
      if (o.checkpoint_every > 0 && !o.checkpoint_path.empty() && r.depth % o.checkpoint_every == 0 && s.level_count > 0) {
        if (int rc = drain_hoist(s, err)) return rc;
        if (int rc = save_checkpoint(o.checkpoint_path, r, s.level_begin, s.level_count, err)) return rc;
      }
    }
    if (int rc = drain_hoist(s, err)) return rc;
    if (prof_ && prof_acc_[3])
      std::fprintf(stderr, "orig_probe per workgroup (us): %.2f  (%llu workgroups)\n",
                   prof_acc_[1] / 100.0 / prof_acc_[3], (unsigned long long)prof_acc_[3]);
    if (prof_) std::fprintf(stderr, "max concurrent dedup workgroups %llu\n", (unsigned long long)prof_acc_[4]);
    for (auto& x : prof_acc_) x = 0;
    finish(r, s.t0);
    return 0;
  }

  // The seen-set the search begins on, cleared: the starter (ensure_starter's comment) with the
  // full table's clear queued beside it, or the full table; a recovered search re-inserts every
  // stored state first, so it starts on the full table.
  int begin_search(const RunOpts& o, Search& s, std::string& err) {
    s.full_mask = s.fifo ? table_mask_ : 2 * (table_mask_ + 1) - 1;
    // a run that returned early on the starter may have left the full table's clear in flight
    HIPCHK(hipStreamSynchronize(clear_stream_));
    if (o.recover_path.empty()) {
      if (s.full_mask + 1 >= STARTER_FACTOR * STARTER_SLOTS) s.st_slots = STARTER_SLOTS;
      if (const char* sv = std::getenv("RAFTMC_STARTER_SLOTS")) {
        char* end = nullptr;
        const unsigned long long v = std::strtoull(sv, &end, 0);
        if (end != sv && *end == 0 && (v & (v - 1)) == 0 && (v == 0 || (v >= 64 && v <= (1ull << 32)))) s.st_slots = v;
      }
    }
    s.tbl = d_table_; s.tmask = s.full_mask;
    if (s.st_slots) {
      if (int rc = ensure_starter(s.st_slots, err)) return rc;
      // the starter's clear first, alone: beside the full clear it gets only its share of the
      // bandwidth and ends when that one does (measured: 1.03 ms for 256 MiB beside 4 GiB).  The
      // full clear starts behind it (ctr_ev_ is free until the first level's readback).
      HIPCHK(hipMemsetAsync(d_starter_, 0, s.st_slots * (s.fifo ? 16 : 8), stream_));
      HIPCHK(hipEventRecord(ctr_ev_, stream_));
      HIPCHK(hipStreamWaitEvent(clear_stream_, ctr_ev_, 0));
      HIPCHK(hipMemsetAsync(d_table_, 0, (table_mask_ + 1) * 16, clear_stream_));
      HIPCHK(hipEventRecord(clear_ev_, clear_stream_));
      s.tbl = d_starter_; s.tmask = s.st_slots - 1;
    } else {
      HIPCHK(hipMemsetAsync(d_table_, 0, (table_mask_ + 1) * 16, stream_));
      HIPCHK(hipStreamSynchronize(stream_));
    }
    run_table_ = s.tbl; run_mask_ = s.tmask;
    ctr_clean_ = false;
    // the hoisted pair's counters start every run at orig_reset_ctr's values (clear_stream_, where a
    // run that returned early would have left a hoisted generate, is idle: waited for above)
    hipLaunchKernelGGL(orig_reset_ctr, dim3(1), dim3(64), 0, stream_, (unsigned long long*)d_ctr2_);
    HIPCHK(hipGetLastError());
    return 0;
  }

  // Level 0: the checkpoint's frontier (TLC -recover), or Init (raft_original.tla:139-159), one
  // state, generated and distinct.  ended: Init is outside the model or violates an invariant.
  int init_level0(const RunOpts& o, Search& s, RunResult& r, bool& ended, std::string& err) {
    if (!o.recover_path.empty()) return load_checkpoint(o.recover_path, s.fifo, s, r, s.level_begin, s.level_count, ended, err);
    W s0; S::init(s0);
    u32 w0[S::NW]; S::pack(s0, w0);
    InitWords<NWP> wp = {}; for (int q = 0; q < S::NW; ++q) wp.w[q] = w0[q];
    const u64 fp0 = m_.rt.symmetry ? S::fp_sym(s0, r.seed) : fp64(w0, r.seed);
    static_assert(NWP <= 64, "orig_init_state: one lane per state word");
    if (s.fifo) hipLaunchKernelGGL((orig_init_state<NWP, 2>), dim3(1), dim3(64), 0, stream_, wp, store_.states(), store_.meta(), s.tbl, s.tmask, fp0);
    else hipLaunchKernelGGL((orig_init_state<NWP, 1>), dim3(1), dim3(64), 0, stream_, wp, store_.states(), store_.meta(), s.tbl, s.tmask, fp0);
    HIPCHK(hipGetLastError());
    r.generated = 1; r.distinct = 1; store_.set_total(1);
    r.levels.push_back({1, 1, 0.0});
    r.depth = 1;
    const u32 bad = SS::violated(s0, m_.rt.invariants);
    ended = !S::in_model(s0, m_.rt) || bad;
    if (ended) HIPCHK(hipStreamSynchronize(stream_));   // the run ends here
    if (!S::in_model(s0, m_.rt)) { err = "the initial state violates a state constraint"; r.verdict = MC_VERDICT_OK; r.distinct = 0; return 0; }
    if (bad) {
      r.verdict = MC_VERDICT_INVARIANT_VIOLATION; r.violated = first_violated(bad);
      r.trace.push_back({"<Initial predicate>", state_text(s0, true)});
      finish(r, s.t0);
    }
    return 0;
  }

  // The device keeps what the search still reads (the frontier) and writes (the next level);
  // when the next level, predicted from the last growth ratio with a 1.5x margin, might not fit
  // behind what is stored, the completed levels move to host memory.
  int maybe_spill(Search& s, const RunResult& r, std::string& err) {
    if (s.level_begin <= store_.base() || s.last) return 0;
    const double prev = r.levels.size() >= 2 ? (double)r.levels[r.levels.size() - 2].states : 1.0;
    const double pred = (double)s.level_count * std::max(1.0, (double)s.level_count / std::max(prev, 1.0)) * 1.5;
    if ((double)(store_.total() - store_.base()) + pred <= (double)store_.cap()) return 0;
    // a hoisted generate reads the store by device index: it is given up before anything moves
    if (int rc = drain_hoist(s, err)) return rc;
    if (progress_) std::fprintf(stderr, "spilling %llu completed states to host memory\n", (unsigned long long)(s.level_begin - store_.base()));
    return store_.spill(s.level_begin, s.level_count, stream_, progress_, err);
  }

  // The search stays on the starter while the states so far plus all this level can insert
  // (level_count * NI successors) keep it at most half full, so the starter never reports a
  // full table.  Otherwise the seen-set moves to the full table before the level is queued:
  // the stream waits for the clear (no host wait) and orig_migrate re-inserts the entries.
  int maybe_switch_to_full_table(Search& s, const RunResult& r, std::string& err) {
    if (s.tbl != d_starter_ || s.level_end() + s.level_count * (u64)S::NI <= s.st_slots / 2) return 0;
    HIPCHK(hipStreamWaitEvent(stream_, clear_ev_, 0));
    unsigned long long* const moved = progress_ ? (unsigned long long*)d_stop_ : nullptr;
    if (moved) HIPCHK(hipMemsetAsync(d_stop_, 0, 8, stream_));
    const unsigned mblk = (unsigned)std::min<u64>(2048, (s.st_slots + BS - 1) / BS);
    if (s.fifo) hipLaunchKernelGGL((orig_migrate<2>), dim3(mblk), dim3(BS), 0, stream_, (const u64*)d_starter_, s.st_slots, d_table_, s.full_mask, (unsigned long long*)d_ctr_, moved);
    else hipLaunchKernelGGL((orig_migrate<1>), dim3(mblk), dim3(BS), 0, stream_, (const u64*)d_starter_, s.st_slots, d_table_, s.full_mask, (unsigned long long*)d_ctr_, moved);
    HIPCHK(hipGetLastError());
    if (moved) {
      u64 n = 0;
      HIPCHK(hipMemcpyAsync(&n, d_stop_, 8, hipMemcpyDeviceToHost, stream_));
      HIPCHK(hipStreamSynchronize(stream_));
      std::fprintf(stderr, "seen-set switch after level %lld: %llu entries moved from the %llu-slot starter to the full table\n",
                   (long long)r.depth, (unsigned long long)n, (unsigned long long)s.st_slots);
    }
    s.tbl = d_table_; s.tmask = s.full_mask;
    run_table_ = s.tbl; run_mask_ = s.tmask;
    return 0;
  }

  // Every chunk's kernels are queued without waiting: the chunk's insert and winner counts stay on
  // the device (grid-stride / scanned offsets), so the host synchronises once per level, for the
  // counters (read_level).  Chunk q of the level uses the pool's events 8q .. 8q+7: generate
  // (e0, e1), the seen-set pass (e1 or e2, e3), mark + scan (e3, e5; FIFO only), materialize (e5
  // or e3, e7); kernel boundaries share an event (each event record costs ~5 us of stream time).
  //
  // Generate beside dedup: a large level of the -workers N search is cut into
  // sub-chunks that alternate between the two halves of the record buffers (chunk_plan.h).
  // orig_generate + orig_generate_lead of sub-chunk c + 1 (vector ALU) run on clear_stream_ beside
  // orig_dedup_plain + orig_materialize_plain of sub-chunk c (random HBM probes) on stream_.  All
  // edges are stream waits on events recorded before the wait is queued (a wait on a
  // never-recorded event is a no-op); the host still waits once per level:
  //   first generate of the level  <- gen_ev_: orig_reset_ctr, orig_migrate (and, in stream order
  //                                   on clear_stream_, the full table's clear)
  //   dedup(c)                     <- e[1] of c: orig_generate_lead(c) done
  //   generate(c + 2)              <- e[3] of c: dedup(c) has read the half's records; K_LEAD is
  //                                   re-armed on the generate stream itself, behind lead(c + 1)
  //   counter readback             <- stream_ order: the last materialize, which waited for the
  //                                   last generate, which is behind every earlier one
  // Behind a level hoist (launch_hoist, s.cur) chunk 0 has its records already: no generate is queued
  // for it, its dedup waits for the hoisted lead's event, and the gen_ev_ edge (orig_reset_ctr,
  // orig_fold_ctr, orig_migrate) is chunk 1's, the level's first generate into d_ctr_.
  int queue_level(const RunOpts& o, Search& s, RunResult& r, std::string& err) {
    s.ovl = s.plan.plan(s.level_count, chunks_, s.cur.count, s.cur.buffer);
    const int nchunks = (int)chunks_.size();
    if (s.cur.count && !nchunks) { err = "level hoist: the generated prefix does not fit the level"; return MC_E_STATE; }
    if (!s.ovl || nchunks < 2) s.arm = false;
    const int first_gen = s.cur.count ? 1 : 0;   // chunk 0 of a level behind a hoist has its records already
    hipStream_t const gst = s.ovl ? clear_stream_ : stream_;
    for (s.nch = 0; s.nch < nchunks; ++s.nch) {
      const int q = s.nch;
      const u64 cb = s.level_begin + chunks_[q].first, cnt = chunks_[q].count;
      const u64 rec0 = chunks_[q].buffer ? s.plan.half_cap : 0;
      const unsigned nblk = (unsigned)((cnt + BS - 1) / BS);
      hipEvent_t e[8];
      for (int j = 0; j < 8; ++j) e[j] = pool_ev(8 * q + j);
      if (!e[7]) { err = "hipEventCreate failed"; return MC_E_NO_DEVICE; }
      // kernels index the device store (global id - store_.base()); keys and parent pointers are global
      const GenArgs g = gen_args(cb - store_.base(), cnt, cb, r.seed, o, rec0);
      hipEvent_t gen_done = e[1];
      // (gen_ev_ before anything of the level is on stream_: behind a hoist, chunk 1's generate runs
      // beside chunk 0's dedup)
      if (s.ovl && q == 0) HIPCHK(hipEventRecord(gen_ev_, stream_));
      if (q < first_gen) {
        gen_done = hoist_ev_[s.cur.slot][1];
      } else {
        if (s.ovl && q == first_gen) HIPCHK(hipStreamWaitEvent(gst, gen_ev_, 0));
        if (s.ovl && q >= 2) HIPCHK(hipStreamWaitEvent(gst, pool_ev(8 * (q - 2) + 3), 0));
        HIPCHK(hipEventRecord(e[0], gst));
        launch_generate(g, nblk, gst);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(e[1], gst));
        // K_LEAD for the next sub-chunk's generate, in order behind this one's lead kernel (not
        // after the level's last: orig_reset_ctr does that, and a late zeroing here could hit the
        // next level's count)
        if (s.ovl && q + 1 < nchunks) HIPCHK(hipMemsetAsync(d_ctr_ + K_LEAD, 0, 8, gst));
      }
      if (s.ovl) {
        HIPCHK(hipStreamWaitEvent(stream_, gen_done, 0));
        HIPCHK(hipEventRecord(e[2], stream_));   // dedup's own start: e[1] is the other stream's
      }
      // the seen-set pass, then the store pass: each one sequence per search order.  Beside a generate
      // (every pipelined sub-chunk but the level's last, and that one before a hoist) the -workers N probes run at 4 workgroups per
      // CU, not 8, with 2 probes in flight per thread, not 4: see launch_dedup_plain
      const DedupArgs d = dedup_args(g, cb, s.tbl, s.tmask);
      if (s.fifo) { if (int rc = queue_merge_probe(s, d, nblk, err)) return rc; }
      else launch_dedup_plain(d, nblk, s.ovl && (q + 1 < nchunks || s.arm), s.count_probes);
      HIPCHK(hipGetLastError());
      HIPCHK(hipEventRecord(e[3], stream_));
      if (s.fifo) { if (int rc = queue_winners_materialize(s, cb, cnt, nblk, e[5], err)) return rc; }
      else launch_materialize_plain(mat_plain_args(store_.base(), s.level_end() - store_.base(), !s.last), cnt);
      HIPCHK(hipGetLastError());
      HIPCHK(hipEventRecord(e[7], stream_));
      // between chunks; after the level's last chunk the host adds the two counters it reads back
      // anyway (both paths leave the chunk's count in K_CHUNK_NEW: orig_dedup_plain / orig_scan)
      if (q + 1 < nchunks) {
        hipLaunchKernelGGL(orig_advance, dim3(1), dim3(64), 0, stream_, (unsigned long long*)d_ctr_, s.ovl ? 0 : 1);
        HIPCHK(hipGetLastError());
        // K_LEVEL_NEW is final from here on: what launch_hoist reads
        if (s.arm && q + 2 == nchunks) HIPCHK(hipEventRecord(x_ev_, stream_));
      }
      for (size_t k = 0; k < r.kernels.size(); ++k) if (s.fifo || k != 2) r.kernels[k].launches += 1;
      r.kernels[0].algo_bytes += (double)cnt * NWP * 4;        // + G_in * 10 record bytes per level (read_level)
    }
    return 0;
  }

  // The level hoist: the next level's first generate beside this level's last dedup.
  // orig_generate touches neither the seen-set nor the level's counters' meaning: it needs its
  // parents in the store and a free half of the record buffers, and both are there before the level
  // ends.  With the whole level queued (s.arm: queue_level launched the last dedup in its
  // beside-generate form and recorded x_ev_ behind orig_advance of sub-chunk k - 2) the host reads
  // K_LEVEL_NEW as that kernel left it: X new states of sub-chunks 0 .. k - 2 are stored from
  // level_end on and nothing changes the word again.  The 8-byte copy runs on a stream of its own, so
  // it queues behind neither dedup(k - 1) nor generate(k - 1); the device has all the level's work
  // already.  Then, on the generate stream:
  //   hoisted generate  <- e[7] of k - 2: its states are stored, its half's records have been read
  //                        (stream order: behind generate(k - 1), the half's other user is k - 2)
  // over parents [level_end, level_end + X0) into the half sub-chunk k - 1 does not use, counting into
  // d_ctr2_, so this level's readback sees nothing of the next level (fold_hoist adds the block in
  // at the next level's start), timed by events of its own (the pool's belong to this level).  Every
  // kernel argument is the host's; a hoist under s.hoist_min parents is not worth its launch.
  int launch_hoist(const RunOpts& o, Search& s, RunResult& r, std::string& err) {
    const int k = (int)chunks_.size();
    HIPCHK(hipStreamWaitEvent(x_stream_, x_ev_, 0));
    HIPCHK(hipMemcpyAsync(h_x_, d_ctr_ + K_LEVEL_NEW, 8, hipMemcpyDeviceToHost, x_stream_));
    HIPCHK(hipEventRecord(hx_ev_, x_stream_));
    HIPCHK(hipEventSynchronize(hx_ev_));
    // whole workgroups, one half at the most, and only slots the store has (a full store ends the
    // search at this level's readback)
    const u64 dev0 = s.level_end() - store_.base();
    const u64 room = store_.cap() > dev0 ? store_.cap() - dev0 : 0;
    const u64 x0 = std::min<u64>(std::min<u64>(*h_x_, room), s.plan.half_cap) / BS * BS;
    if (x0 < s.hoist_min) return 0;
    typename Search::Hoist h;
    h.count = x0; h.buffer = chunks_[k - 1].buffer ^ 1; h.slot = s.cur.slot ^ 1;
    GenArgs g = gen_args(dev0, x0, s.level_end(), r.seed, o, h.buffer ? s.plan.half_cap : 0);
    g.ctr = (unsigned long long*)d_ctr2_;
    HIPCHK(hipStreamWaitEvent(clear_stream_, pool_ev(8 * (k - 2) + 7), 0));
    HIPCHK(hipEventRecord(hoist_ev_[h.slot][0], clear_stream_));
    launch_generate(g, (unsigned)(x0 / BS), clear_stream_);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(hoist_ev_[h.slot][1], clear_stream_));
    s.next = h;
    if (progress_)
      std::fprintf(stderr, "level hoist: %llu parents of level %lld generated beside the last dedup of level %lld\n",
                   (unsigned long long)x0, (long long)r.depth + 1, (long long)r.depth);
    return 0;
  }

  // level start behind a hoist (s.cur): the hoisted pair's counters into the level's, behind
  // orig_reset_ctr (stream order) and the pair itself
  int fold_hoist(const Search& s, std::string& err) {
    if (!s.cur.count) return 0;
    HIPCHK(hipStreamWaitEvent(stream_, hoist_ev_[s.cur.slot][1], 0));
    hipLaunchKernelGGL(orig_fold_ctr, dim3(1), dim3(64), 0, stream_, (unsigned long long*)d_ctr_, (unsigned long long*)d_ctr2_);
    HIPCHK(hipGetLastError());
    return 0;
  }

  // Every way out of the level loop but the next level's queue_level comes through here first: a
  // queued hoist (s.next) is waited for and forgotten, its counters are reset, and the generate stream
  // and both halves are free for whatever follows (a FIFO re-search, a spill, a checkpoint, the next
  // run of the handle).
  int drain_hoist(Search& s, std::string& err) {
    if (!s.next.count) return 0;
    s.next = typename Search::Hoist();
    HIPCHK(hipStreamSynchronize(clear_stream_));
    hipLaunchKernelGGL(orig_reset_ctr, dim3(1), dim3(64), 0, stream_, (unsigned long long*)d_ctr2_);
    HIPCHK(hipGetLastError());
    return 0;
  }

  // a chunk's seen-set pass in TLC's single-worker order: the records merged per workgroup, then probed
  int queue_merge_probe(const Search& s, const DedupArgs& d, unsigned nblk, std::string& err) {
    hipLaunchKernelGGL(orig_merge, dim3(nblk), dim3(BS), 0, stream_, d);
    HIPCHK(hipGetLastError());
    if (s.count_probes) hipLaunchKernelGGL((orig_probe<true>), dim3(nblk), dim3(BS), 0, stream_, d);
    else hipLaunchKernelGGL((orig_probe<false>), dim3(nblk), dim3(BS), 0, stream_, d);
    return 0;
  }

  // its store pass: the winners among the inserted records (mark, count, scan; e5 behind them),
  // then their states in key order
  int queue_winners_materialize(const Search& s, u64 cb, u64 cnt, unsigned nblk, hipEvent_t e5, std::string& err) {
    MarkArgs mk;
    mk.newpos = d_newrec_; mk.table = s.tbl; mk.gid0 = cb; mk.chunk_count = cnt; mk.winmask = d_winmask_;
    mk.ww = WW; mk.ctr = (unsigned long long*)d_ctr_;
    hipLaunchKernelGGL(orig_mark, dim3((unsigned)std::min<u64>(2048, (cnt * 2 + BS - 1) / BS)), dim3(BS), 0, stream_, mk);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL((orig_count<WW>), dim3(nblk), dim3(BS), 0, stream_, (const u64*)d_winmask_, cnt, d_wcnt_);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(orig_scan, dim3(1), dim3(SCAN_BS), 0, stream_, (const u32*)d_wcnt_, d_woff_, (u32)nblk, (unsigned long long*)d_ctr_);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e5, stream_));
    MatArgs m;
    m.states = store_.states(); m.meta = store_.meta(); m.chunk_begin = cb - store_.base(); m.chunk_count = cnt; m.gid0 = cb;
    m.winmask = d_winmask_; m.woff = d_woff_; m.ww = WW; m.dst_base = s.level_end() - store_.base(); m.cap = store_.cap();
    m.rt = m_.rt; m.ctr = (unsigned long long*)d_ctr_;
    if (safety()) hipLaunchKernelGGL((orig_materialize<SS>), dim3(nblk), dim3(BS), 0, stream_, m);
    else hipLaunchKernelGGL((orig_materialize<S>), dim3(nblk), dim3(BS), 0, stream_, m);
    return 0;
  }

  // The level's one host wait: the counters (left in h_ctr_), then the event times, the progress
  // line, and the per-kernel accounting; s.nnew and s.level_ms are the level's.
  int read_level(Search& s, RunResult& r, std::string& err) {
    u64* const c = h_ctr_;   // pinned: the readback is one direct copy
    HIPCHK(hipMemcpyAsync(c, d_ctr_, K_NCTR * 8, hipMemcpyDeviceToHost, stream_));
    HIPCHK(hipEventRecord(ctr_ev_, stream_));
    hipLaunchKernelGGL(orig_reset_ctr, dim3(1), dim3(64), 0, stream_, (unsigned long long*)d_ctr_);
    HIPCHK(hipGetLastError());
    ctr_clean_ = true;
    // the host waits for the copy alone (the level's kernel events were all recorded before it):
    // the reset behind it runs while the host looks at the counters
    HIPCHK(hipEventSynchronize(ctr_ev_));
    const bool fifo = s.fifo, last = s.last;
    const u64 level_end = s.level_end(), S_B = NWP * 4;
    double level_ms = 0;
    for (int q = 0; q < s.nch; ++q) {
      // event pairs per kernel (queue_level); dedup starts at e2 on a pipelined level, where e1 is
      // the generate stream's.  On a pipelined level the pairs time kernels that share the device:
      // their sum exceeds the time the device was busy.
      const std::pair<int, int> pr[4] = {{0, 1}, {s.ovl ? 2 : 1, 3}, {3, fifo ? 5 : 3}, {fifo ? 5 : 3, 7}};
      for (int k = 0; k < 4; ++k) {
        float ms = 0;
        // (chunk 0 behind a hoist: its generate ran in the level before, timed by the hoist's own pair)
        if (k == 0 && q == 0 && s.cur.count) (void)hipEventElapsedTime(&ms, hoist_ev_[s.cur.slot][0], hoist_ev_[s.cur.slot][1]);
        else if (pr[k].first != pr[k].second) (void)hipEventElapsedTime(&ms, pool_ev(8 * q + pr[k].first), pool_ev(8 * q + pr[k].second));
        r.kernels[k].ms += ms; level_ms += ms;
      }
    }
    const u64 nnew = c[K_LEVEL_NEW] + c[K_CHUNK_NEW];   // earlier chunks (orig_advance) + the last one
    const u64 next_write = level_end + nnew;
    if (progress_)   // TLC's progress line, per BFS level (RAFTMC_PROGRESS=1), on stderr
      std::fprintf(stderr, "Progress(%lld) at %.3f s: %lld states generated, %llu distinct states found, %llu states left on queue "
                           "(level kernels %.1f ms, %d chunk(s), store %llu/%llu, %llu on the host%s)\n",
                   (long long)r.depth + 1,
                   std::chrono::duration<double>(std::chrono::steady_clock::now() - s.t0).count(),
                   (long long)(r.generated + (int64_t)[&] { u64 g = 0; for (int k = 0; k < OA_NACT; ++k) g += c[K_ACT + k]; return g; }()),
                   (unsigned long long)(level_end + nnew), (unsigned long long)nnew, level_ms, s.nch,
                   (unsigned long long)((last ? level_end : next_write) - store_.base()), (unsigned long long)store_.cap(), (unsigned long long)store_.base(),
                   last ? "; the last level counted, not stored" : "");
    if (progress_ && (c[K_EVENT] != ~0ull || c[K_ERR]))
      std::fprintf(stderr, "level %lld: event word 0x%llx, error flags 0x%llx\n", (long long)r.depth + 1,
                   (unsigned long long)c[K_EVENT], (unsigned long long)c[K_ERR]);
    if (prof_) {
      for (int q = 0; q < 4; ++q) prof_acc_[q] += c[K_PROF + q];
      prof_acc_[4] = std::max<u64>(prof_acc_[4], c[K_PROF + 5]);
    }
    const u64 G_in = c[K_GEN_IN];
    // per-kernel algorithmic bytes: generate writes 10-B records; dedup reads them and probes
    // (8 B per in-model successor) and writes 16 B per new state; mark reads the
    // inserted positions + keys and sets winner bits; materialize re-reads the parent and writes
    // state + parent pointer
    r.kernels[0].algo_bytes += (double)G_in * 10;
    r.kernels[1].algo_bytes += (double)G_in * (10 + 8) + (double)nnew * (16 + 8);
    r.kernels[2].algo_bytes += (double)nnew * (8 + 16 + 8);
    r.kernels[3].algo_bytes += (double)s.level_count * WW * 8 + (double)nnew * (S_B + S_B + 8);
    r.seconds_kernels += level_ms / 1000.0;
    r.n_launches += 1;
    s.nnew = nnew; s.level_ms = level_ms;
    return 0;
  }

  // TLC -workers N found an event: TLC's counterexample and stop point are the single-worker
  // search's, so the model is searched again in FIFO order (it stops at this level)
  int research_fifo(const RunOpts& o, u64 evw, RunResult& r, std::string& err) {
    RunOpts o1 = o;
    o1.workers = 1;
    o1.recover_path.clear();        // a checkpoint of this search is in its order, not TLC's: start over
    o1.checkpoint_path.clear();
    const int64_t ev_depth = r.depth + 1;
    const int rc = run(o1, r, err);
    if (rc == 0 && r.verdict == MC_VERDICT_CAPACITY_OVERFLOW) {
      // the FIFO re-search stores every level (count_final_level included): when it does not
      // fit, the event the -workers N pass found is still reported, not lost
      static const char* const kind[4] = {"an evaluation error", "a deadlock", "an invariant evaluation error", "an invariant or action property violation"};
      r.error = std::string("the -workers N search found ") + kind[evw & 3] + " at depth " + std::to_string(ev_depth) +
                "; TLC's single-worker re-search of it (for TLC's counterexample and stop point) ran out of capacity: " + r.error;
    }
    return rc;
  }

  // the text of a capacity verdict: c = the level's counters, whose K_ERR is not 0
  std::string capacity_error(const u64* c, u64 level_end, u64 nnew, int64_t depth) const {
    const u64 e = c[K_ERR];
    std::ostringstream os;
    os << "error flags 0x" << std::hex << e << std::dec << " while expanding state " << (c[K_ERRGID] ? (int64_t)(c[K_ERRGID] - 1) : -1) << ":";
    if (e & OE_CAP_ELECTIONS) os << " elections set exceeds the compiled capacity;";
    if (e & OE_CAP_COUNT) os << " message count / bag capacity exceeded;";
    if (e & OE_CAP_STORE)
      os << " state store full (raise state_store_bytes): " << store_.cap() << " state slots, " << store_.base()
         << " states on the host, level ends at " << level_end << ", " << nnew << " new;";
    if (e & OE_TABLE_FULL) os << " fingerprint table full (raise fp_table_bytes);";
    // the summary counts the completed levels (their sizes sum to it, and the depth is theirs);
    // whatever part of the interrupted level reached the store is not a level of the search
    os << " the summary counts the " << level_end << " states of the " << depth << " completed levels;";
    return os.str();
  }

  // TLC's stop point at the level's first event (key order = TLC's single-worker FIFO order):
  // generated = whole successor lists of the parents before the event's parent and of the
  // parent itself (none when computing its successors raised the error); per-action generated
  // stops at the event's successor; distinct = states inserted before it (the level's new
  // states are stored in key order: a binary search over their parent pointers); left on queue
  // = the level's parents after it + the new states found before it.
  // stored: how many of the level's nnew new states the store holds (a prefix in key order);
  // decided = false when the event may lie behind states the full store cut off
  int handle_event(u64 ev, u64 level_begin, u64 level_count, u64 nnew, u64 stored, bool inv_oom, RunResult& r, bool& decided,
                   std::string& err) {
    const int kind = (int)(ev & 3);
    const u64 key = ev >> 2, pg = key >> 8;
    const u32 k = (u32)(key & 255);
    const u64 level_end = level_begin + level_count;
    // distinct: this level's new states with key < event key (<= for a violation: the violating
    // state itself is new when it is in the model)
    auto key_at = [&](u64 i, u64& kk) -> int {
      u64 mt = 0;
      HIPCHK(hipMemcpy(&mt, store_.meta() + (level_end - store_.base()) + i, 8, hipMemcpyDeviceToHost));
      kk = ((mt >> 24) << 8) | (mt & 0xff);
      return 0;
    };
    u64 lo = 0, hi = stored;   // first index whose key is beyond the stop point
    while (lo < hi) {
      const u64 mid = (lo + hi) / 2;
      u64 kk = 0;
      if (int rc = key_at(mid, kk)) return rc;
      const bool before = kk < key || (kk == key && kind >= EV_INV_ERROR);
      if (before) lo = mid + 1; else hi = mid;
    }
    const u64 before = lo;
    decided = before < stored || stored == nnew;
    const auto te0 = std::chrono::steady_clock::now();
    auto since = [&]() { return std::chrono::duration<double>(std::chrono::steady_clock::now() - te0).count(); };
    if (progress_)
      std::fprintf(stderr, "event kind %d at parent %llu instance %u: %llu new states before it (%s)\n", kind,
                   (unsigned long long)pg, k, (unsigned long long)before, decided ? "decided" : "beyond the stored states");
    if (!decided) return 0;
    (void)nnew;
    // generated (device: re-derive the successor lists of the level's parents up to pg)
    HIPCHK(hipMemsetAsync(d_stop_, 0, (1 + OA_NACT) * 8, stream_));
    const u64 npar = pg - level_begin + 1;
    hipLaunchKernelGGL((orig_stop_generated<S>), dim3((unsigned)((npar + BS - 1) / BS)), dim3(BS), 0, stream_,
                       (const u32*)store_.states(), level_begin - store_.base(), npar, level_begin, pg, k, (u32)kind, (unsigned long long*)d_stop_);
    HIPCHK(hipGetLastError());
    u64 gs[1 + OA_NACT];
    HIPCHK(hipMemcpyAsync(gs, d_stop_, sizeof gs, hipMemcpyDeviceToHost, stream_));
    HIPCHK(hipStreamSynchronize(stream_));
    HIPCHK(hipMemsetAsync(d_stop_, 0, (1 + OA_NACT) * 8, stream_));
    if (before)
      hipLaunchKernelGGL(orig_stop_distinct, dim3((unsigned)((before + BS - 1) / BS)), dim3(BS), 0, stream_,
                         (const u64*)(store_.meta() + (level_end - store_.base())), before, (unsigned long long*)d_stop_);
    HIPCHK(hipGetLastError());
    u64 ds[1 + OA_NACT];
    HIPCHK(hipMemcpyAsync(ds, d_stop_, sizeof ds, hipMemcpyDeviceToHost, stream_));
    HIPCHK(hipStreamSynchronize(stream_));
    if (progress_) std::fprintf(stderr, "stop-point counters over %llu parents: %.3f s\n", (unsigned long long)npar, since());
    r.generated += (int64_t)gs[0];
    for (int a = 0; a < OA_NACT; ++a) { r.act_generated[a] += (int64_t)gs[1 + a]; r.act_distinct[a] += (int64_t)ds[a]; }
    r.distinct = (int64_t)(level_end + before);
    r.left_on_queue = (int64_t)(level_end - pg - 1 + before);
    // the event's parent and (for a violation) successor, re-derived on the host
    u32 w[NWP]; u64 meta = 0;
    if (!store_.read(pg, w, &meta)) { err = "event state readback failed"; return MC_E_NO_DEVICE; }
    W s; S::unpack(w, s);
    if (kind == EV_NEXT_ERROR) {
      r.verdict = MC_VERDICT_EVAL_ERROR;
      r.error = "TLC evaluation error while computing the successors of state " + std::to_string(pg) +
                ": log[i][prevLogIndex] applied outside its domain (raft_original.tla:207-210)";
      build_trace(pg, nullptr, s, r, err);
      return 0;
    }
    if (kind == EV_DEADLOCK) {
      r.verdict = MC_VERDICT_DEADLOCK;
      build_trace(pg, nullptr, s, r, err);
      return 0;
    }
    W t;
    const int act = successor(s, (int)k, t);
    name_violation(s, t, (int)k, inv_oom, r.verdict, r.violated);
    r.depth += 1;
    build_trace(pg, act >= 0 ? kOrigActNames[act] : "?", t, r, err);
    if (progress_) std::fprintf(stderr, "trace of %zu states: %.3f s\n", r.trace.size(), since());
    return 0;
  }

  // ---------------------------------------------------------------- checkpoint / recover
  // ckpt::OrigHead around the shared framing (ckpt_file.h) and store body (state_store.h)
  int save_checkpoint(const std::string& path, const RunResult& r, u64 level_begin, u64 level_count, std::string& err) {
    const std::string desc = describe_json();
    ckpt::OrigHead h;
    std::memcpy(h.magic, "RAFTMCK2", 8);
    h.fifo = last_fifo_ ? 1 : 0;
    h.nwp = NWP; h.total = store_.total(); h.level_begin = level_begin; h.level_count = level_count;
    ckpt_of_run(r, desc, h);
    return ckpt::write_file(path, h, desc, r.act_generated, r.act_distinct, r.levels, [&](FILE* f) { return store_.write_body(f); }, err);
  }
  // the rank files of a multi-GPU search (ckpt_file.h): this rank's store as it is,
  // parent pointers rank-tagged; levels: this rank's states of every level of sres_
  int save_rank_file(const std::string& path, std::string& err) {
    const std::string desc = describe_json();
    ckpt::ShardHead h;
    std::memset(&h, 0, sizeof h);
    std::memcpy(h.magic, ckpt::kRankMagic, 8);
    h.nwp = NWP; h.total = store_.total(); h.level_begin = sh_level_begin_; h.level_count = sh_level_count_;
    h.rank = rank_; h.world = world_; h.generation = sres_.depth;
    ckpt_of_run(sres_, desc, h);
    std::vector<ckpt::LevelRow> rows(sres_.levels.size());
    if (sh_levels_.size() != rows.size()) { err = "checkpoint: this rank's level table is incomplete"; return MC_E_STATE; }
    for (size_t l = 0; l < rows.size(); ++l) rows[l] = {(int64_t)sh_levels_[l], sres_.levels[l].states};
    return ckpt::write_file(ckpt::rank_path(path, h.generation, rank_), h, desc, sres_.act_generated, sres_.act_distinct, rows,
                            [&](FILE* f) { return store_.write_body(f); }, err);
  }
  // ... and, by rank 0 once every rank file is complete, the manifest; the rank files it replaces go last
  int save_manifest(const std::string& path, std::string& err) {
    const std::string desc = describe_json();
    ckpt::ShardHead h, old;
    std::memset(&h, 0, sizeof h);
    std::memset(&old, 0, sizeof old);
    std::memcpy(h.magic, ckpt::kManifestMagic, 8);
    h.nwp = NWP; h.total = (u64)sres_.distinct; h.level_count = (u64)sres_.levels.back().states; h.level_begin = h.total - h.level_count;
    h.rank = -1; h.world = world_; h.generation = sres_.depth;
    ckpt_of_run(sres_, desc, h);
    {   // the manifest this one replaces names the rank files to remove
      const ckpt::File f = ckpt::open_file(path, "rb");
      if (!f || std::fread(&old, sizeof old, 1, f.get()) != 1 || std::memcmp(old.magic, ckpt::kManifestMagic, 8) != 0) old.world = 0;
    }
    if (int rc = ckpt::write_file(path, h, desc, sres_.act_generated, sres_.act_distinct, sres_.levels, [](FILE*) { return true; }, err)) return rc;
    ckpt::remove_stale_rank_files(path, old.generation, old.world, h.generation, h.world);
    return 0;
  }

  // ---------------------------------------------------------------- recovery at any GPU count
  // (orig_reshard.hip)  What rank `me` of `world` holds once the source is in its store:
  struct Resharded {
    std::vector<u64> local;   // its states of every level
    u64 total = 0;            // ... of all levels
    bool overflow = false;    // its share does not fit its store (nothing was written behind the end)
  };
  // Reads the whole source level by level in the canonical order, in blocks through one pinned
  // bounce buffer, and places this rank's share in store_ (states from slot 0, levels one behind the
  // other).  Kernel times go to sres_.kernels[k0] (classify) and [k0 + 1] (place).  The seen-set is
  // not touched.  A parent pointer that names no state of the level before: MC_E_INVALID.
  int reshard_load(const ckpt::ShardSource& src, int me, int world, int k0, Resharded& out, std::string& err) {
    const int SW = src.world;
    const size_t nl = src.levels.size();
    u64 max_level = 0, max_slice = 0;
    for (size_t l = 0; l < nl; ++l) {
      max_level = std::max<u64>(max_level, (u64)src.levels[l].states);
      for (int r = 0; r < SW; ++r) max_slice = std::max<u64>(max_slice, src.parts[r].level_count[l]);
    }
    const u64 block = std::min<u64>(StateStore::kBlock, max_slice), nwg_max = (block + BS - 1) / BS;
    struct Tmp {   // freed on every way out
      u32* st = nullptr; u64* me = nullptr; unsigned char* own = nullptr; u32* cnt = nullptr; u64* off = nullptr;
      u64* map0 = nullptr; u64* map1 = nullptr; u64* run = nullptr;
      u32* h_st = nullptr; u64* h_me = nullptr;
      DevOwner<HipDevApi> res;
    } t;
    HIPCHK(t.res.device(&t.st, block * NWP * 4));
    HIPCHK(t.res.device(&t.me, block * 8));
    HIPCHK(t.res.device(&t.own, block));
    HIPCHK(t.res.device(&t.cnt, nwg_max * RESHARD_MAX_WORLD * 4));
    HIPCHK(t.res.device(&t.off, nwg_max * RESHARD_MAX_WORLD * 8));
    HIPCHK(t.res.device(&t.map0, max_level * 8));
    HIPCHK(t.res.device(&t.map1, max_level * 8));
    HIPCHK(t.res.device(&t.run, (RESHARD_MAX_WORLD + 1) * 8));
    HIPCHK(t.res.pinned(&t.h_st, block * NWP * 4));
    HIPCHK(t.res.pinned(&t.h_me, block * 8));
    // two read positions per part: its states and its parent pointers, both in level order
    std::vector<ckpt::File> fs, fm;
    for (int r = 0; r < SW; ++r) {
      const ckpt::SourcePart& p = src.parts[r];
      fs.push_back(ckpt::open_file(p.path, "rb"));
      fm.push_back(ckpt::open_file(p.path, "rb"));
      if (!fs[r] || !fm[r] || std::fseek(fs[r].get(), (long)p.body, SEEK_SET) != 0 ||
          std::fseek(fm[r].get(), (long)(p.body + p.total * NWP * 4), SEEK_SET) != 0) {
        err = "cannot read checkpoint " + p.path;
        return MC_E_IO;
      }
    }
    HIPCHK(hipMemsetAsync(d_ctr_ + K_ERR, 0, 8, stream_));
    ReshardPlaceArgs a;
    std::memset(&a, 0, sizeof a);
    a.me = (u32)me; a.states = store_.states(); a.meta = store_.meta(); a.cap = store_.cap(); a.ctr = (unsigned long long*)d_ctr_;
    a.in_states = t.st; a.in_meta = t.me; a.owner = t.own; a.wg_off = t.off;
    a.map_prev = t.map1; a.map_cur = t.map0;
    ReshardLevel cur;
    std::memset(&cur, 0, sizeof cur);
    double read_s = 0;
    out = Resharded();
    for (size_t l = 0; l < nl; ++l) {
      cur.world = (u32)SW;
      for (int r = 0; r < SW; ++r) { cur.begin[r] += l ? src.parts[r].level_count[l - 1] : 0; cur.count[r] = src.parts[r].level_count[l]; }
      a.level_size = reshard_canonical(cur);
      HIPCHK(hipMemsetAsync(t.run, 0, RESHARD_MAX_WORLD * 8, stream_));
      a.pos0 = 0;
      for (int r = 0; r < SW; ++r) {
        for (u64 b = 0; b < cur.count[r]; b += block) {
          const u64 n = std::min<u64>(block, cur.count[r] - b);
          const auto tr = std::chrono::steady_clock::now();
          if (std::fread(t.h_st, 4, n * NWP, fs[r].get()) != n * NWP || std::fread(t.h_me, 8, n, fm[r].get()) != n) {
            err = "checkpoint " + src.parts[r].path + " is truncated";
            return MC_E_IO;
          }
          read_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - tr).count();
          HIPCHK(hipMemcpyAsync(t.st, t.h_st, n * NWP * 4, hipMemcpyHostToDevice, stream_));
          HIPCHK(hipMemcpyAsync(t.me, t.h_me, n * 8, hipMemcpyHostToDevice, stream_));
          const unsigned nwg = (unsigned)((n + BS - 1) / BS);
          a.n = n;
          if (int rc = timed(k0, [&] {
                hipLaunchKernelGGL((orig_reshard_classify<S>), dim3(nwg), dim3(BS), 0, stream_, (const u32*)t.st, n, (u64)src.seed, (u32)world, t.own, t.cnt);
                hipLaunchKernelGGL(orig_reshard_scan, dim3(1), dim3(BS), 0, stream_, (const u32*)t.cnt, (u32)nwg, t.run, t.off);
              }, err)) return rc;
          if (int rc = timed(k0 + 1, [&] { hipLaunchKernelGGL((orig_reshard_place<NWP>), dim3(nwg), dim3(BS), 0, stream_, a); }, err)) return rc;
          HIPCHK(hipStreamSynchronize(stream_));   // the bounce buffer is free again
          harvest();
          sres_.kernels[k0].algo_bytes += (double)n * (NWP * 4 + 1);
          sres_.kernels[k0 + 1].algo_bytes += (double)n * (8 + 1 + 8) + (double)n / world * (2.0 * NWP * 4 + 8);
          a.pos0 += n;
        }
      }
      u64 h[RESHARD_MAX_WORLD + 1];   // the level's states per owner, and the error word
      HIPCHK(hipMemcpyAsync(t.run + RESHARD_MAX_WORLD, d_ctr_ + K_ERR, 8, hipMemcpyDeviceToDevice, stream_));
      HIPCHK(hipMemcpyAsync(h, t.run, sizeof h, hipMemcpyDeviceToHost, stream_));
      HIPCHK(hipStreamSynchronize(stream_));
      u64 sum = 0;
      for (int o = 0; o < RESHARD_MAX_WORLD; ++o) sum += h[o];
      if ((h[RESHARD_MAX_WORLD] & OE_RESHARD_PARENT) || sum != a.level_size) {
        err = "checkpoint " + src.parts[0].path + " is not a checkpoint of this model (a parent pointer of level " + std::to_string(l + 1) +
              " names no state of the level before)";
        return MC_E_INVALID;
      }
      out.local.push_back(h[me]);
      out.total += h[me];
      if (out.total > store_.cap()) { out.overflow = true; break; }
      for (int o = 0; o < RESHARD_MAX_WORLD; ++o) a.owner_begin[o] += h[o];
      a.prev = cur; a.prev_size = a.level_size;
      u64* const done_map = a.map_cur;
      a.map_cur = const_cast<u64*>(a.map_prev); a.map_prev = done_map;
    }
    HIPCHK(hipMemsetAsync(d_ctr_ + K_ERR, 0, 8, stream_));
    HIPCHK(hipStreamSynchronize(stream_));
    if (progress_)
      std::fprintf(stderr, "recover: rank %d of %d read %zu levels of %d part(s): file read %.3f s, classify %.3f ms, place %.3f ms\n", me, world, nl,
                   SW, read_s, sres_.kernels[k0].ms, sres_.kernels[k0 + 1].ms);
    return 0;
  }
  // the seen-set of a -workers N search (8-B entries) from this rank's n stored states; full: the table is
  int reshard_reinsert(u64 n, u64 seed, int k, bool& full, std::string& err) {
    full = false;
    if (n) {
      if (int rc = timed(k, [&] {
            hipLaunchKernelGGL((orig_reinsert<S, 1>), dim3((unsigned)((n + BS - 1) / BS)), dim3(BS), 0, stream_, (const u32*)store_.states(), n, d_table_,
                               2 * table_mask_ + 1, seed, (unsigned long long*)d_ctr_);
          }, err)) return rc;
      sres_.kernels[k].algo_bytes += (double)n * (NWP * 4 + 8);
    }
    u64 e = 0;
    HIPCHK(hipMemcpyAsync(&e, d_ctr_ + K_ERR, 8, hipMemcpyDeviceToHost, stream_));
    HIPCHK(hipStreamSynchronize(stream_));
    harvest();
    full = e != 0;
    HIPCHK(hipMemsetAsync(d_ctr_ + K_ERR, 0, 8, stream_));
    return 0;
  }
  static void run_of_source(const ckpt::ShardSource& src, RunResult& r) {
    r.seed = src.seed; r.generated = src.generated; r.distinct = src.distinct; r.depth = src.depth; r.generated_in_model = src.generated_in_model;
    r.act_generated = src.act_generated; r.act_distinct = src.act_distinct;
    r.levels.clear();
    for (const auto& lv : src.levels) r.levels.push_back({lv.states, lv.generated, 0.0});
  }
  // the text of a recovery whose share did not fit: r holds the source's counters
  static std::string reshard_full_error(const RunResult& r, int world, u64 cap) {
    return "state store full (raise state_store_bytes or recover on more GPUs): the checkpoint's " + std::to_string(r.distinct) +
           " states do not fit " + std::to_string(world) + " store(s) of " + std::to_string(cap) +
           " slots (a recovery from a multi-GPU checkpoint or at another GPU count does not spill to the host); the summary counts the " +
           std::to_string(r.distinct) + " states of the " + std::to_string(r.depth) + " completed levels;";
  }

  // mc_run on one GPU from a multi-GPU checkpoint: W' = 1 of the path above into the single-GPU store.
  // ended: the file does not fit the device store (CAPACITY_OVERFLOW: this path has no host spill)
  int load_resharded(const std::string& path, bool fifo, const Search& s, RunResult& r, u64& level_begin, u64& level_count, bool& ended,
                     std::string& err) {
    if (fifo) {
      err = "checkpoint " + path + " was written by a multi-GPU search, a -workers N search: its kept parents are not TLC's single-worker "
            "FIFO ones, so it cannot resume a -workers 1 search";
      return MC_E_INVALID;
    }
    ckpt::ShardSource src;
    if (int rc = ckpt::open_source(path, NWP, OA_NACT, describe_json(), src, err)) return rc;
    sres_ = new_result(src.seed, {"orig_reshard_classify", "orig_reshard_place", "orig_reinsert"});
    pending_.clear();
    Resharded got;
    if ((u64)src.distinct <= store_.cap())
      if (int rc = reshard_load(src, 0, 1, 0, got, err)) return rc;
    run_of_source(src, r);
    if ((u64)src.distinct > store_.cap() || got.overflow) {
      r.verdict = MC_VERDICT_CAPACITY_OVERFLOW;
      r.error = reshard_full_error(r, 1, store_.cap());
      store_.set_total(0);
      finish(r, s.t0);
      ended = true;
      return 0;
    }
    bool full = false;
    if (int rc = reshard_reinsert(got.total, src.seed, 2, full, err)) return rc;
    if (full) { err = "fingerprint table too small for the checkpoint (raise fp_table_bytes)"; return MC_E_OOM; }
    for (const auto& k : sres_.kernels) r.kernels.push_back(k);
    store_.set_total(got.total);
    level_count = got.local.back(); level_begin = got.total - level_count;
    return 0;
  }

  int load_checkpoint(const std::string& path, bool fifo, const Search& s, RunResult& r, u64& level_begin, u64& level_count, bool& ended,
                      std::string& err) {
    HIPCHK(hipMemsetAsync(d_ctr_, 0, K_NCTR * 8, stream_));
    if (ckpt::file_magic(path) == ckpt::kManifestMagic) return load_resharded(path, fifo, s, r, level_begin, level_count, ended, err);
    ckpt::OrigHead h;
    ckpt::Reader in(path);
    if (int rc = in.head("RAFTMCK2", NWP, OA_NACT, describe_json(), h, r.act_generated, r.act_distinct, r.levels, err)) return rc;
    if (fifo && !h.fifo) {
      err = "checkpoint " + path + " was written by a -workers N search: its kept parents are not TLC's single-worker "
            "FIFO ones, so it cannot resume a -workers 1 search";
      return MC_E_INVALID;
    }
    auto reinsert = [&](const u32* states, u64 n) {
      const dim3 grid((unsigned)((n + BS - 1) / BS));
      if (m_.rt.symmetry && last_fifo_)
        hipLaunchKernelGGL((orig_reinsert_sym<S, 2>), grid, dim3(BS), 0, stream_, states, n, d_table_, table_mask_, (u64)h.seed, (unsigned long long*)d_ctr_);
      else if (m_.rt.symmetry)
        hipLaunchKernelGGL((orig_reinsert_sym<S, 1>), grid, dim3(BS), 0, stream_, states, n, d_table_, 2 * table_mask_ + 1, (u64)h.seed, (unsigned long long*)d_ctr_);
      else if (last_fifo_)
        hipLaunchKernelGGL((orig_reinsert<S, 2>), grid, dim3(BS), 0, stream_, states, n, d_table_, table_mask_, (u64)h.seed, (unsigned long long*)d_ctr_);
      else
        hipLaunchKernelGGL((orig_reinsert<S, 1>), grid, dim3(BS), 0, stream_, states, n, d_table_, 2 * table_mask_ + 1, (u64)h.seed, (unsigned long long*)d_ctr_);
    };
    // the host part's fingerprints go in through the (idle) candidate buffer, chunk by chunk
    const u64 stage = std::max<u64>(1, chunk_states_ * S::NI * 8 / (NWP * 4));
    if (int rc = store_.read_body(in, h.total, h.level_begin, d_rfp_, stage, stream_, d_ctr_ + K_ERR, reinsert, err)) return rc;
    run_of_ckpt(h, r);
    level_begin = h.level_begin; level_count = h.level_count;
    return 0;
  }

  int dump_states(const std::string& path, std::string& err) override {
    if (!store_.states()) { err = "mc_dump_states before mc_run"; return MC_E_STATE; }
    if (unstored_) { err = "mc_dump_states: the last level was counted, not stored (count_final_level)"; return MC_E_STATE; }
    return rmc::dump_states<NWP>(store_, path, [&](const u32 (&w)[NWP]) { return words_text(w, false); }, err);
  }

  // ================================================================ sharded mode
  int shard_open(const RunOpts& o, int rank, int world, std::string& err) override {
    if (world < 1 || world > 8 || rank < 0 || rank >= world) { err = "sharded mode supports 1..8 ranks"; return MC_E_INVALID; }
    if (m_.rt.symmetry) { err = "SYMMETRY for raft_original runs on one GPU (mc_run); the sharded search has no orbit fingerprints"; return MC_E_UNSUPPORTED; }
    if (int rc = ensure_alloc(o, world, err)) return rc;
    rank_ = rank; world_ = world; sopts_ = o;
    unstored_ = 0;
    last_fifo_ = false;   // 8-B entries (observed_collision)
    HIPCHK(hipMemsetAsync(d_table_, 0, (table_mask_ + 1) * 16, stream_));
    HIPCHK(hipMemsetAsync(d_ctr_, 0, K_NCTR * 8, stream_));
    HIPCHK(hipMemsetAsync(d_ctr_ + K_EVENT, 0xFF, 8, stream_));
    HIPCHK(hipStreamSynchronize(stream_));
    sres_ = new_result(bfs_seed(o), {"orig_generate", "orig_route_blk", "orig_dedup_sh", "orig_materialize_sh", "orig_store"});
    pending_.clear();
    st0_ = std::chrono::steady_clock::now();
    // Init: one state, stored and inserted by the owner of its fingerprint
    W s0; S::init(s0);
    u32 w0[S::NW]; S::pack(s0, w0);
    const u64 fp0 = fp64(w0, sres_.seed);
    store_.set_total(0); sh_level_begin_ = 0; sh_level_count_ = 0; sh_new_ = 0;
    store_.reset();
    sh_levels_.assign(1, 0);
    // (a recovering search takes its first levels from the checkpoint: shard_run_native, shard_recover)
    if (o.recover_path.empty() && (int)fp_owner(fp0, (u32)world) == rank) {
      u32 wp[NWP] = {0}; for (int q = 0; q < S::NW; ++q) wp[q] = w0[q];
      HIPCHK(hipMemcpy(d_table_ + (fp0 & sh_table_mask()), &fp0, 8, hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(store_.states(), wp, NWP * 4, hipMemcpyHostToDevice));
      const u64 nometa = ~0ull;
      HIPCHK(hipMemcpy(store_.meta(), &nometa, 8, hipMemcpyHostToDevice));
      store_.set_total(1); sh_level_count_ = 1; sh_levels_[0] = 1;
    }
    sres_.generated = 1; sres_.distinct = 1; sres_.depth = 1;
    sres_.levels.push_back({1, 0, 0.0});
    if (!S::in_model(s0, m_.rt)) { err = "the initial state violates a state constraint"; return MC_E_UNSUPPORTED; }
    if (SS::violated(s0, m_.rt.invariants)) { err = "the initial state violates an invariant"; return MC_E_UNSUPPORTED; }
    sh_next_write_ = store_.total();
    return 0;
  }
  u64 sh_table_mask() const { return 2 * table_mask_ + 1; }   // sharded seen-set: 8-B entries
  int shard_record_bytes(int what) const override {
    return what == MC_SHARD_ROUTE ? 16 : what == MC_SHARD_REPLY ? 8 : what == MC_SHARD_STATES ? (NWP + 4) * 4 : -1;
  }
  int shard_frontier(int64_t* states, int64_t* chunk) const override {
    if (states) *states = (int64_t)sh_level_count_;
    if (chunk) *chunk = (int64_t)chunk_states_;
    return 0;
  }
  // ---- the step API: each step queues one stage, waits for it and counts as one launch of its
  // kernel, however many segments the stage launched
  int shard_generate(int64_t begin, int64_t count, int64_t* counts, std::string& err) override {
    if (begin < 0 || count < 0 || (u64)count > chunk_states_ || (u64)(begin + count) > sh_level_count_) { err = "shard_generate: chunk outside the frontier"; return MC_E_INVALID; }
    sh_chunk_begin_ = sh_level_begin_ + (u64)begin; sh_chunk_count_ = (u64)count;
    if (int rc = stage_generate_route(err)) return rc;
    u64 c[8] = {0};
    HIPCHK(hipMemcpyAsync(c, d_rcnt_, 8 * 8, hipMemcpyDeviceToHost, stream_));
    HIPCHK(hipStreamSynchronize(stream_));
    harvest();
    if (count > 0) {
      u64 valid = 0; for (int r = 0; r < world_; ++r) valid += c[r];
      sres_.kernels[1].algo_bytes += (double)valid * 16;
    }
    for (int r = 0; r < world_; ++r) { counts[r] = (int64_t)c[r]; fill_counts_route_[r] = c[r]; }
    return 0;
  }

  int shard_fill(int what, void* dst, const int64_t* offsets, std::string& err) override {
    const int rb = shard_record_bytes(what);
    if (rb < 0) { err = "shard_fill: bad record kind"; return MC_E_INVALID; }
    for (int r = 0; r < world_; ++r) {
      u64 n = 0;
      const char* src = nullptr;
      if (what == MC_SHARD_ROUTE) { n = fill_counts_route_[r]; src = (const char*)(d_route_ + (u64)r * chunk_states_ * S::NI * 2); }
      else if (what == MC_SHARD_REPLY) { n = fill_counts_reply_[r]; src = (const char*)(d_newrec_ + seg_off_[r]); }
      else { n = fill_counts_states_[r]; src = (const char*)(d_stout_ + seg_off_ack_[r] * (NWP + 4)); }
      if (n && !dst) { err = "shard_fill: null destination for a non-empty segment"; return MC_E_INVALID; }
      if (n) HIPCHK(hipMemcpyAsync((char*)dst + (u64)offsets[r] * rb, src, n * rb, hipMemcpyDeviceToDevice, stream_));
    }
    HIPCHK(hipStreamSynchronize(stream_));
    return 0;
  }

  int shard_dedup(const void* recv, const int64_t* counts, int64_t* reply_counts, std::string& err) override {
    Seg seg[8];
    u64 total = 0;
    for (int r = 0; r < world_; ++r) { seg[r] = {(const u64*)recv + 2 * total, (u64)counts[r]}; total += (u64)counts[r]; }
    if (total > chunk_states_ * S::NI) { err = "shard_dedup: received more records than one chunk holds"; return MC_E_INVALID; }
    auto& kd = sres_.kernels[2];
    const int64_t steps = kd.launches + 1;
    if (int rc = stage_dedup(seg, err)) return rc;
    u64 c[8] = {0};
    HIPCHK(hipMemcpyAsync(c, d_rcnt_ + 8, 8 * 8, hipMemcpyDeviceToHost, stream_));
    HIPCHK(hipStreamSynchronize(stream_));
    harvest();
    u64 nnew = 0;
    for (int r = 0; r < world_; ++r) { reply_counts[r] = (int64_t)c[r]; fill_counts_reply_[r] = c[r]; nnew += c[r]; }
    kd.launches = steps; kd.algo_bytes += (double)total * 24 + (double)nnew * 16;
    return 0;
  }

  int shard_materialize(const void* acks, const int64_t* counts, std::string& err) override {
    Seg ack[8];
    u64 total = 0;
    for (int r = 0; r < world_; ++r) { ack[r] = {(const u64*)acks + total, (u64)counts[r]}; total += (u64)counts[r]; fill_counts_states_[r] = (u64)counts[r]; }
    auto& km = sres_.kernels[3];
    const int64_t steps = km.launches + 1;
    if (int rc = stage_rederive(ack, false, -1, 0, err)) return rc;
    HIPCHK(hipStreamSynchronize(stream_));
    harvest();
    km.launches = steps;
    return 0;
  }

  int shard_store(const void* states, int64_t n, std::string& err) override {
    if (n <= 0) return 0;
    if (int rc = stage_store((const u32*)states, (u64)n, err)) return rc;
    HIPCHK(hipStreamSynchronize(stream_));
    harvest();
    return 0;
  }

  int shard_level_stats(int64_t* st, std::string& err) override {
    u64 c[K_NCTR];
    HIPCHK(hipMemcpy(c, d_ctr_, sizeof c, hipMemcpyDeviceToHost));
    std::memset(st, 0, MC_SHARD_NSTAT * sizeof(int64_t));
    st[0] = (int64_t)sh_new_;
    int64_t gen = 0;
    for (int k = 0; k < OA_NACT; ++k) { st[8 + k] = (int64_t)c[K_ACT + k]; st[40 + k] = (int64_t)c[K_ACT + OA_NACT + k]; gen += (int64_t)c[K_ACT + k]; }
    st[1] = gen; st[2] = (int64_t)c[K_GEN_IN];
    // the sharded raft_original search is not FIFO-ranked across ranks: any event stops it
    sh_event_ = c[K_EVENT];
    const int kind = sh_event_ == ~0ull ? -1 : (int)(sh_event_ & 3);
    st[3] = (int64_t)(c[K_ERR] | (sh_next_write_ > store_.cap() ? (u64)OE_CAP_STORE : 0ull) | (kind == EV_NEXT_ERROR ? (u64)OE_EVAL_LOG_INDEX : 0ull));
    // [4] is max-reduced over the ranks: 2 = an invariant, 1 = an action property (orig_spec.h §14) -- TLC
    // checks invariants before implied actions, so an invariant on any rank names the stop
    sviol_act_.clear(); sviol_verdict_ = 0;
    if (kind == EV_VIOLATION) {
      // this rank's violating step, re-derived from (parent, instance)
      const u64 key = sh_event_ >> 2, par = key >> 8;
      const int k = (int)(key & 255);
      u32 w[NWP];
      HIPCHK(hipMemcpy(w, store_.states() + par * NWP, NWP * 4, hipMemcpyDeviceToHost));
      W s, t; S::unpack(w, s);
      const int act = successor(s, k, t);
      name_violation(s, t, k, sopts_.inv_out_of_model, sviol_verdict_, sviol_name_);
      sviol_parent_ = ((u64)rank_ << 37) | par; sviol_act_ = act >= 0 ? kOrigActNames[act] : "?";
      sviol_text_ = state_text(t, true);
    }
    st[4] = kind != EV_VIOLATION ? 0 : sviol_verdict_ == MC_VERDICT_ACTION_PROPERTY_VIOLATION ? 1 : 2;
    st[5] = kind == EV_DEADLOCK ? 1 : 0; st[6] = (int64_t)sh_level_count_;
    return 0;
  }

  int shard_level_commit(const int64_t* g, int* done, std::string& err) override {
    sres_.generated += g[1];
    sres_.generated_in_model += g[2];
    for (int k = 0; k < OA_NACT; ++k) { sres_.act_generated[k] += g[8 + k]; sres_.act_distinct[k] += g[40 + k]; }
    sres_.levels.back().generated = g[1];
    *done = 0;
    if (g[3]) {
      sres_.verdict = (g[3] & (OE_CAP_STORE | OE_TABLE_FULL | OE_CAP_ELECTIONS | OE_CAP_COUNT)) ? MC_VERDICT_CAPACITY_OVERFLOW : MC_VERDICT_EVAL_ERROR;
      sh_event_ = ~0ull;
      std::ostringstream os; os << "error flags 0x" << std::hex << g[3] << " raised on some rank"; sres_.error = os.str();
      *done = 1;
    }
    if (*done && sres_.verdict == MC_VERDICT_CAPACITY_OVERFLOW) {
      // as on one GPU: the summary counts the completed levels; the interrupted one is not a level
      sres_.error += "; the summary counts the " + std::to_string(sres_.distinct) + " states of the " +
                     std::to_string(sres_.depth) + " completed levels";
    } else {
      sres_.distinct += g[0];
      if (g[0] > 0) { sres_.levels.push_back({g[0], 0, 0.0}); sres_.depth += 1; sh_levels_.push_back(sh_new_); }
    }
    if (!*done && g[4]) {
      sres_.verdict = g[4] == 1 ? MC_VERDICT_ACTION_PROPERTY_VIOLATION : MC_VERDICT_INVARIANT_VIOLATION;
      *done = 1; sres_.left_on_queue = g[0];
    }
    if (!*done && sopts_.check_deadlock && g[5]) { sres_.verdict = MC_VERDICT_DEADLOCK; *done = 1; sres_.left_on_queue = g[0]; }
    if (!*done && g[0] == 0) *done = 1;
    if (!*done && sopts_.max_depth && sres_.depth >= sopts_.max_depth) { sres_.verdict = MC_VERDICT_DEPTH_LIMIT; sres_.left_on_queue = g[0]; *done = 1; }
    // advance the local level
    sh_level_begin_ += sh_level_count_;
    sh_level_count_ = sh_new_;
    store_.set_total(sh_next_write_);
    sh_new_ = 0;
    HIPCHK(hipMemset(d_ctr_, 0, K_NCTR * 8));
    HIPCHK(hipMemset(d_ctr_ + K_EVENT, 0xFF, 8));
    sres_.n_launches += 1;
    if (*done) {
      // this rank's violating step (shard_level_stats derived it) counts when it is of the kind the
      // ranks agreed on
      const bool viol = sres_.verdict == MC_VERDICT_INVARIANT_VIOLATION || sres_.verdict == MC_VERDICT_ACTION_PROPERTY_VIOLATION;
      if (!viol || sh_event_ == ~0ull || sviol_verdict_ != sres_.verdict) sviol_act_.clear();
      if (viol) sres_.violated = sviol_act_.empty() ? "" : sviol_name_;
      double secs = 0; for (auto& k : sres_.kernels) secs += k.ms / 1000.0;
      sres_.seconds_kernels = secs;
      finish(sres_, st0_);
    }
    return 0;
  }

  int shard_read_state(uint64_t gid, std::string& text, uint64_t* meta, std::string& err) const override {
    const u64 local = gid & ((1ull << 37) - 1);
    if (!store_.states()) { err = "shard_read_state: the device memory of this handle was released"; return MC_E_STATE; }
    if (local >= store_.total()) { err = "shard_read_state: state id outside this rank's store"; return MC_E_INVALID; }
    u32 w[NWP]; u64 m = 0;
    if (!store_.read(local, w, &m)) { err = "readback failed"; return MC_E_NO_DEVICE; }
    W s; S::unpack(w, s);
    text = state_text(s, true);
    if (meta) *meta = m;
    return 0;
  }
  int shard_violation(uint64_t* parent, std::string& action, std::string& text) const override {
    if (parent) *parent = sviol_parent_;
    action = sviol_act_; text = sviol_text_;
    return sviol_act_.empty() ? MC_E_STATE : 0;
  }
  const RunResult* shard_result() const override { return &sres_; }

  // ---------------------------------------------------------------- native level loop
  // The whole sharded BFS of raft-tla_amd/shard.py (sharded_bfs) in C++ on one HIP stream:
  // per chunk generate+route -> counts exchange -> ROUTE payload -> dedup -> counts exchange ->
  // REPLY payload -> materialize -> STATES payload -> store, over a ShardTransport
  // (shard_transport.h: grouped ncclSend/ncclRecv straight from the kernels' buffers between
  // GPUs, or the in-process loopback of mc_shard_run_loopback) with two host synchronisations
  // per chunk (the counts) plus one per level (the all-reduce of the level statistics).
  int shard_run_native(ShardTransport& T, std::string& err) override {
    const int W = world_, me = rank_;
    const u64 SBW = (u64)(NWP + 4) * 4;          // STATES record bytes
    if (!d_nat_) HIPCHK(res_.device(&d_nat_, (32 + 2 * MC_SHARD_NSTAT) * 8));
    if (!h_nat_) HIPCHK(res_.pinned(&h_nat_, (32 + 2 * MC_SHARD_NSTAT) * 8));
    u64* d_xs = d_nat_;        // [0,8) counts I send  (copied from d_rcnt_)
    u64* d_xr = d_nat_ + 8;    // [8,16) counts I receive
    int64_t* d_sum = (int64_t*)(d_nat_ + 32);
    int64_t* d_max = d_sum + MC_SHARD_NSTAT;
    u64* h_xs = h_nat_; u64* h_xr = h_nat_ + 8;
    int64_t* h_sum = (int64_t*)(h_nat_ + 32);
    int64_t* h_max = h_sum + MC_SHARD_NSTAT;
    // counts exchange: send[r] from d_send (device), received into d_xr; both land on the host
    auto xcounts = [&](const u64* d_send) -> int {
      HIPCHK(hipMemcpyAsync(d_xs, d_send, 8 * (u64)W, hipMemcpyDeviceToDevice, stream_));
      HIPCHK(hipMemcpyAsync(d_xr + me, d_send + me, 8, hipMemcpyDeviceToDevice, stream_));
      if (W > 1) {
        const char* src[8]; char* dst[8]; u64 n8[8];
        for (int r = 0; r < W; ++r) { src[r] = (const char*)(d_xs + r); dst[r] = (char*)(d_xr + r); n8[r] = 8; }
        if (T.exchange(me, W, src, n8, dst, n8, stream_, err)) return MC_E_NO_DEVICE;
      }
      HIPCHK(hipMemcpyAsync(h_xs, d_xs, 16 * 8, hipMemcpyDeviceToHost, stream_));
      HIPCHK(hipStreamSynchronize(stream_));
      return 0;
    };
    // payload exchange: segment r of the send side (bytes) goes to rank r, the receive side is
    // packed in source-rank order; the self segment is not copied (its consumer reads it in
    // place), so dst + roff[me] stays unused
    auto xpay = [&](const char* const* src, const u64* sbytes, char* dst, const u64* rbytes) -> int {
      char* dsts[8]; u64 acc = 0;
      for (int r = 0; r < W; ++r) { dsts[r] = dst + acc; acc += rbytes[r]; }
      if (sbytes[me] != rbytes[me]) { err = "sharded exchange: self segment size mismatch"; return MC_E_STATE; }
      if (W > 1 && T.exchange(me, W, src, sbytes, dsts, rbytes, stream_, err)) return MC_E_NO_DEVICE;
      return 0;
    };
    auto allreduce_level = [&](int64_t* g, int64_t next_chunks, int64_t& chunks_out) -> int {
      // g: local stats in, global stats out; MAX slots: [3,6) flags, [6] chunk rounds of the next
      // level, [8, 8+32) one slot per bit of the error word (max per bit = bitwise OR over ranks:
      // two ranks' different capacity errors are both reported)
      static_assert(8 + 32 <= MC_SHARD_NSTAT, "max slots");
      for (int k = 0; k < MC_SHARD_NSTAT; ++k) h_sum[k] = g[k];
      for (int k = 0; k < MC_SHARD_NSTAT; ++k) h_max[k] = 0;
      h_max[3] = g[3]; h_max[4] = g[4]; h_max[5] = g[5]; h_max[6] = next_chunks;
      for (int b = 0; b < 32; ++b) h_max[8 + b] = (g[3] >> b) & 1;
      HIPCHK(hipMemcpyAsync(d_sum, h_sum, 2 * MC_SHARD_NSTAT * 8, hipMemcpyHostToDevice, stream_));
      if ((W > 1 || T.allreduce_at_world1()) && T.allreduce(d_sum, MC_SHARD_NSTAT, d_max, 8 + 32, stream_, err)) return MC_E_NO_DEVICE;
      HIPCHK(hipMemcpyAsync(h_sum, d_sum, 2 * MC_SHARD_NSTAT * 8, hipMemcpyDeviceToHost, stream_));
      HIPCHK(hipStreamSynchronize(stream_));
      for (int k = 0; k < MC_SHARD_NSTAT; ++k) g[k] = h_sum[k];
      g[3] = 0;
      for (int b = 0; b < 32; ++b) g[3] |= (h_max[8 + b] ? 1ll : 0ll) << b;
      g[4] = h_max[4]; g[5] = h_max[5];
      chunks_out = h_max[6];
      return 0;
    };

    const u64 chunk = chunk_states_;
    auto rounds = [&](u64 n) -> int64_t { return (int64_t)((n + chunk - 1) / chunk); };
    int64_t nchunks = 0;
    int64_t start_flags = 0;   // a recovered share that does not fit this rank's store or seen-set
    if (!sopts_.recover_path.empty())
      if (int rc = shard_recover(start_flags, err)) return rc;
    {   // agree on the first level's chunk rounds (only the owner of Init holds a state)
      int64_t z[MC_SHARD_NSTAT] = {0};
      z[3] = start_flags;
      if (int rc = allreduce_level(z, rounds(sh_level_count_), nchunks)) return rc;
      start_flags = z[3];
    }
    if (start_flags || (!sopts_.recover_path.empty() && sopts_.max_depth && sres_.depth >= sopts_.max_depth)) {
      // the recovered search ends before its first level: some rank's share did not fit, or the
      // checkpoint already is as deep as this run may go
      if (start_flags) {
        sres_.verdict = MC_VERDICT_CAPACITY_OVERFLOW;
        std::ostringstream os; os << "error flags 0x" << std::hex << start_flags << " raised on some rank while recovering: ";
        sres_.error = os.str() + ((start_flags & OE_CAP_STORE) ? reshard_full_error(sres_, world_, store_.cap()) : std::string("fingerprint table full (raise fp_table_bytes);"));
      } else {
        sres_.verdict = MC_VERDICT_DEPTH_LIMIT;
        sres_.left_on_queue = sres_.levels.back().states;
      }
      sviol_act_.clear();
      finish(sres_, st0_);
      return 0;
    }
    // TLC -checkpoint on W GPUs: every rank its own file, then, once all of them are
    // complete, rank 0 the manifest; a rank that could not write stops every rank
    auto checkpoint = [&]() -> int {
      std::string werr;
      int wrc = save_rank_file(sopts_.checkpoint_path, werr);
      int64_t z[MC_SHARD_NSTAT] = {0}, unused = 0;
      z[3] = wrc ? 1 : 0;
      if (int rc = allreduce_level(z, 0, unused)) return rc;
      if (!z[3] && me == 0) wrc = save_manifest(sopts_.checkpoint_path, werr);
      if (z[3] && !wrc) { wrc = MC_E_IO; werr = "writing checkpoint " + sopts_.checkpoint_path + " failed on another rank"; }
      if (wrc) err = werr;
      return wrc;
    };
    const u64 route_cap = chunk_states_ * S::NI;
    // count_final_level: the level at depth max_depth is never expanded, so its new states are
    // deduplicated by their owners, counted and invariant-checked by the generating rank, but
    // neither shipped to the owners nor stored (no STATES exchange, no store kernel): the ranks'
    // stores hold the levels before it (BASELINE configs[4], C5v2 to depth 14 on 8 GPUs)
    const bool count_last = sopts_.count_final_level && sopts_.max_depth > 0;
    unstored_ = 0;
    for (;;) {
      const u64 front = sh_level_count_;
      const bool last = count_last && sres_.depth + 1 >= sopts_.max_depth;
      if (sopts_.test_fail_rank == me && sopts_.test_fail_depth == sres_.depth) {   // mc_set_fault_injection (tests)
        err = "injected failure (mc_set_fault_injection) at depth " + std::to_string(sres_.depth);
        return MC_E_STATE;
      }
      for (int64_t c = 0; c < nchunks; ++c) {
        const u64 begin = std::min<u64>((u64)c * chunk, front);
        const u64 count = std::min<u64>(chunk, front - begin);
        sh_chunk_begin_ = sh_level_begin_ + begin; sh_chunk_count_ = count;
        if (W == 1) {
          // World 1: every fingerprint is this rank's, so the route pass, both counts exchanges (the
          // chunk's two host synchronisations) and the acknowledged re-derivation collapse into the
          // single-GPU -workers N kernels: orig_dedup_plain's first-come LDS filter is the route's, its
          // probes the owner's, orig_materialize_plain stores the new states behind the level; the
          // counts stay on the device (orig_advance), the host waits once per level
          if (count == 0) continue;
          const unsigned nblk = (unsigned)((count + BS - 1) / BS);
          const GenArgs g = sh_gen_args();
          if (int rc = stage_generate(g, nblk, err)) return rc;
          DedupArgs d = dedup_args(g, sh_chunk_begin_, d_table_, sh_table_mask());
          d.prof = 0;   // (RAFTMC_PROF reads the counters of mc_run's levels only)
          if (int rc = timed(2, [&] { launch_dedup_plain(d, nblk, false, false); }, err)) return rc;
          const MatPlainArgs m = mat_plain_args(0, sh_next_write_, !last);
          if (int rc = timed(3, [&] { launch_materialize_plain(m, count); }, err)) return rc;
          hipLaunchKernelGGL(orig_advance, dim3(1), dim3(64), 0, stream_, (unsigned long long*)d_ctr_, 1);
          HIPCHK(hipGetLastError());
          continue;
        }
        if (int rc = stage_generate_route(err)) return rc;
        // ---- ROUTE: (fp, slot) records to the fingerprints' owners
        if (int rc = xcounts(d_rcnt_)) return rc;
        u64 scnt[8], rcnt[8], sb[8], rb[8], rtot = 0;
        const char* src[8];
        for (int r = 0; r < W; ++r) {
          scnt[r] = h_xs[r]; rcnt[r] = h_xr[r]; rtot += rcnt[r];
          sb[r] = scnt[r] * 16; rb[r] = rcnt[r] * 16;
          src[r] = (const char*)(d_route_ + (u64)r * route_cap * 2);
          sres_.kernels[1].algo_bytes += (double)scnt[r] * 16;
        }
        if (rtot > route_cap) { err = "shard: received more ROUTE records than one chunk holds"; return MC_E_STATE; }
        if (int rc = grow(nat_recv_, nat_recv_cap_, rtot * 16, err)) return rc;
        if (int rc = xpay(src, sb, (char*)nat_recv_, rb)) return rc;
        // ---- owner-side dedup, one launch per source rank (the self segment where route left it)
        Seg seg[8];
        u64 off = 0;
        for (int r = 0; r < W; ++r) {
          seg[r] = {r == me ? d_route_ + (u64)me * route_cap * 2 : (const u64*)nat_recv_ + 2 * off, rcnt[r]};
          off += rcnt[r];
        }
        if (int rc = stage_dedup(seg, err)) return rc;
        // ---- REPLY: the new ones' slots back to the generating ranks
        if (int rc = xcounts(d_rcnt_ + 8)) return rc;
        u64 rep[8], ack[8], atot = 0, ntot = 0;
        for (int r = 0; r < W; ++r) {
          rep[r] = h_xs[r]; ack[r] = h_xr[r]; atot += ack[r]; ntot += rep[r];
          sb[r] = rep[r] * 8; rb[r] = ack[r] * 8;
          src[r] = (const char*)(d_newrec_ + seg_off_[r]);
        }
        sres_.kernels[2].algo_bytes += (double)rtot * 24 + (double)ntot * 16;
        if (int rc = grow(nat_acks_, nat_acks_cap_, atot * 8, err)) return rc;
        if (int rc = xpay(src, sb, (char*)nat_acks_, rb)) return rc;
        // ---- generator re-derives the acknowledged states; my own new ones go into my store
        // after the ones of lower ranks
        u64 before = 0;
        for (int q = 0; q < me; ++q) before += rep[q];
        off = 0;
        for (int r = 0; r < W; ++r) {
          seg[r] = {r == me ? d_newrec_ + seg_off_[me] : (const u64*)nat_acks_ + off, ack[r]};
          off += ack[r];
        }
        if (int rc = stage_rederive(seg, last, me, sh_next_write_ + before, err)) return rc;
        if (last) {   // the owners count their new states of the final level; nothing is shipped
          for (int r = 0; r < W; ++r) sh_new_ += rep[r];
          continue;
        }
        // ---- STATES: packed states + parent pointers to their owners (sizes known: no sync)
        for (int r = 0; r < W; ++r) { sb[r] = ack[r] * SBW; rb[r] = rep[r] * SBW; src[r] = (const char*)(d_stout_ + seg_off_ack_[r] * (NWP + 4)); }
        if (int rc = grow(nat_stin_, nat_stin_cap_, ntot * SBW, err)) return rc;
        if (int rc = xpay(src, sb, (char*)nat_stin_, rb)) return rc;
        // the owner stores the states in source-rank order (its own ones were materialized in place)
        off = 0;
        for (int r = 0; r < W; ++r) {
          if (rep[r] && r == me) { sh_next_write_ += rep[r]; sh_new_ += rep[r]; }
          else if (rep[r])
            if (int rc = stage_store((const u32*)((const char*)nat_stin_ + off * SBW), rep[r], err)) return rc;
          off += rep[r];
        }
      }
      HIPCHK(hipStreamSynchronize(stream_));
      harvest();
      if (W == 1) {   // the level's new states (orig_advance's running count), stored behind the level
        u64 lvl_new = 0;
        HIPCHK(hipMemcpy(&lvl_new, d_ctr_ + K_LEVEL_NEW, 8, hipMemcpyDeviceToHost));
        sh_new_ = lvl_new;
        if (!last) sh_next_write_ += lvl_new;
      }
      int64_t g[MC_SHARD_NSTAT];
      if (int rc = shard_level_stats(g, err)) return rc;
      if (W == 1) {   // SURVEY.md §8(d) bytes of the fused kernels (the W > 1 ones count per exchange)
        sres_.kernels[2].algo_bytes += (double)g[2] * (10 + 8) + (double)sh_new_ * (16 + 8);
        sres_.kernels[3].algo_bytes += (double)sh_new_ * (2.0 * NWP * 4 + 8);
      }
      int64_t next_chunks = 0;
      if (int rc = allreduce_level(g, rounds(sh_new_), next_chunks)) return rc;
      if (last) unstored_ = sh_new_;   // this rank's share of the final level: counted, not in the store
      int done = 0;
      if (int rc = shard_level_commit(g, &done, err)) return rc;
      // as on one GPU: behind every checkpoint_every-th completed level that left a frontier, the
      // level a depth limit stops at included; never behind a level that ended in an error
      if (sopts_.checkpoint_every > 0 && !sopts_.checkpoint_path.empty() && (!done || sres_.verdict == MC_VERDICT_DEPTH_LIMIT) &&
          g[0] > 0 && sres_.depth % sopts_.checkpoint_every == 0)
        if (int rc = checkpoint()) return rc;
      if (done) break;
      nchunks = next_chunks;
    }
    return 0;
  }

  // TLC -recover on W' GPUs: this rank's share of the source (a multi-GPU checkpoint of any world
  // size, or a single-GPU file of either search order) into its store, its seen-set rebuilt, the
  // search's counters the source's.  flags: OE_CAP_STORE / OE_TABLE_FULL when the share does not fit.
  int shard_recover(int64_t& flags, std::string& err) {
    ckpt::ShardSource src;
    if (int rc = ckpt::open_source(sopts_.recover_path, NWP, OA_NACT, describe_json(), src, err)) return rc;
    const int k0 = (int)sres_.kernels.size();
    for (const char* k : {"orig_reshard_classify", "orig_reshard_place", "orig_reinsert"}) sres_.kernels.push_back({k, 0, 0, 0});
    Resharded got;
    if (int rc = reshard_load(src, rank_, world_, k0, got, err)) return rc;
    run_of_source(src, sres_);
    sh_levels_ = got.local;
    if (got.overflow) { flags |= OE_CAP_STORE; sh_levels_.resize(src.levels.size(), 0); got.total = 0; }
    bool full = false;
    if (int rc = reshard_reinsert(got.total, src.seed, k0 + 2, full, err)) return rc;
    if (full) flags |= OE_TABLE_FULL;
    store_.set_total(got.total);
    sh_level_count_ = got.overflow ? 0 : got.local.back(); sh_level_begin_ = got.total - sh_level_count_;
    sh_next_write_ = got.total; sh_new_ = 0;
    return 0;
  }

 private:
  OrigModel m_;
  static constexpr int WW = (S::NI + 63) / 64;   // winner-mask words per parent
  u64* d_table_ = nullptr; u64* d_ctr_ = nullptr; u64* d_stop_ = nullptr;
  u64* h_ctr_ = nullptr;     // pinned host copy of the level counters
  bool ctr_clean_ = false;   // d_ctr_ already reset for the next level (queued after the readback)
  u64* d_rfp_ = nullptr; unsigned short* d_rkey_ = nullptr; u32* d_rcnt_blk_ = nullptr; u64* d_newrec_ = nullptr;
  u64* d_winmask_ = nullptr; u32* d_wcnt_ = nullptr; u64* d_woff_ = nullptr; u64* d_urec_ = nullptr; u32* d_ucnt_ = nullptr;
  u64* d_route_ = nullptr; u64* d_rcnt_ = nullptr;
  u32* d_stout_ = nullptr; u64 stout_cap_ = 0;   // re-derived STATES records (stage_rederive), its bytes
  u32* d_lead_ = nullptr;      // [chunk] the chunk's leader-work parents (orig_generate -> orig_generate_lead)
  hipStream_t stream_ = nullptr;
  hipEvent_t ctr_ev_ = nullptr;          // recorded behind the level's counter readback
  // the starter seen-set (ensure_starter) and the stream / event of the full table's clear
  u64* d_starter_ = nullptr; u64 starter_cap_ = 0;
  hipStream_t clear_stream_ = nullptr; hipEvent_t clear_ev_ = nullptr;
  hipEvent_t gen_ev_ = nullptr;          // pipelined level: stream_ is ready for the level's first generate
  // the level hoist (launch_hoist)
  u64* d_ctr2_ = nullptr; u64* h_x_ = nullptr;
  hipStream_t x_stream_ = nullptr;
  hipEvent_t x_ev_ = nullptr, hx_ev_ = nullptr, hoist_ev_[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
  std::vector<Chunk> chunks_;            // the current level's chunks (chunk_plan.h)
  u64* run_table_ = nullptr; u64 run_mask_ = 0;   // the table the last single-GPU run ended on (entries - 1)
  u64 table_mask_ = 0, chunk_states_ = 0;
  u64 unstored_ = 0;   // states of the last level counted but not stored (count_final_level)
  int dev_ = -1, alloc_world_ = 0; uint64_t req_table_ = 0, req_store_ = 0;
  // sharded-mode state
  int rank_ = 0, world_ = 1;
  RunOpts sopts_;
  RunResult sres_;
  std::chrono::steady_clock::time_point st0_;
  u64 sh_level_begin_ = 0, sh_level_count_ = 0, sh_next_write_ = 0, sh_new_ = 0, sh_chunk_begin_ = 0, sh_chunk_count_ = 0;
  u64 seg_off_[8] = {0}, seg_off_ack_[8] = {0}, fill_counts_reply_[8] = {0}, fill_counts_states_[8] = {0};
  u64 fill_counts_route_[8] = {0};
  u64 sviol_parent_ = 0; int sviol_verdict_ = 0; std::string sviol_act_, sviol_text_, sviol_name_;
  u64 sh_event_ = ~0ull;
  std::vector<u64> sh_levels_;   // this rank's states of every level of sres_.levels (the rank file's level rows)
  bool last_fifo_ = true;   // seen-set layout of the last single-GPU run (16-B keyed / 8-B entries)
  // RAFTMC_PROF=1: per-phase wall-clock ticks (100 MHz) of orig_dedup, summed over workgroups
  const bool prof_ = std::getenv("RAFTMC_PROF") != nullptr;
  const bool progress_ = std::getenv("RAFTMC_PROGRESS") != nullptr;
  u64 prof_acc_[5] = {0, 0, 0, 0, 0};
  // native (RCCL) level loop buffers
  u64* d_nat_ = nullptr; u64* h_nat_ = nullptr;
  void* nat_recv_ = nullptr; void* nat_acks_ = nullptr; void* nat_stin_ = nullptr;
  u64 nat_recv_cap_ = 0, nat_acks_cap_ = 0, nat_stin_cap_ = 0;
  std::vector<int> pending_;   // sharded stages: the kernel of each event pair not yet read back (timed / harvest)
  StateStore store_;   // the stored states and parent pointers: device part + host spill
  // owns every device and pinned allocation, event and stream named above (and the pool of timing
  // events): each is created through it, and release() frees them all
  DevOwner<HipDevApi> res_;

  void release_device() override { release(); }
  void release() {
    // a run that returned early may have left the full table's clear in flight
    if (clear_stream_) (void)hipStreamSynchronize(clear_stream_);
    if (x_stream_) (void)hipStreamSynchronize(x_stream_);
    if (stream_) (void)hipStreamSynchronize(stream_);
    res_.release();   // streams last
    store_.release();
    starter_cap_ = 0; stout_cap_ = 0; nat_recv_cap_ = nat_acks_cap_ = nat_stin_cap_ = 0;
    run_table_ = nullptr; run_mask_ = 0;
    pending_.clear();
    ctr_clean_ = false;
    dev_ = -1; alloc_world_ = 0;   // nothing allocated: the next ensure_alloc starts over
  }

  // successor k of s as the search keeps it (allLogs advanced), and the action that made it (< 0: none)
  static int successor(const W& s, int k, W& t) {
    u64 al[S::AW]; S::all_logs_next(s, al);
    u32 e2 = 0;
    const int act = S::apply(s, k, t, e2);
    for (int q = 0; q < S::AW; ++q) t.allLogs[q] = al[q];
    return act;
  }

  // What a violation event at the step (s, t) of instance k reports: TLC checks the
  // invariants of a successor it is about to keep (new; or out of the model under MC_COMPAT_INV_OUT_OF_MODEL)
  // before the implied actions, so a broken invariant is named first; else the first listed property the
  // step breaks, in cfg order.  (An in-model successor already in the seen-set satisfies every invariant: a
  // state that breaks one stops the search at the key it was found at, which is smaller.)
  void name_violation(const W& s, const W& t, int k, bool inv_oom, int& verdict, std::string& name) const {
    const u32 bad = (S::in_model(t, m_.rt) || inv_oom) ? SS::violated(t, m_.rt.invariants) : 0u;
    if (bad || !actions()) { verdict = MC_VERDICT_INVARIANT_VIOLATION; name = first_violated(bad); return; }
    const u32 pbad = S::violated_action(s, t, k, m_.rt.action_props);
    verdict = MC_VERDICT_ACTION_PROPERTY_VIOLATION;
    name = "?";
    for (auto& n : m_.prop_names)
      if (pbad & orig_prop_bit(n.c_str())) { name = n; break; }
  }

  std::string first_violated(u32 bad) const {
    for (auto& n : m_.inv_names) {
      if (bad & orig_inv_bit(n.c_str())) return n;
    }
    return "?";
  }

  // a parent pointer: the action in bits 16..23, the parent's global id from bit 24 up
  void build_trace(u64 parent, const char* last_act, const W& last, RunResult& r, std::string& err) {
    rmc::build_trace<NWP>(store_, parent, last_act, last_act ? state_text(last, true) : std::string(),
                          [&](const u32 (&w)[NWP]) { return words_text(w, true); }, kOrigActNames, 16, 0xff, 24, r.trace, err);
  }
  std::string words_text(const u32 (&w)[NWP], bool multiline) const { W s; S::unpack(w, s); return state_text(s, multiline); }

  std::string state_text(const W& s, bool multiline) const { return orig_state_text<S>(m_, s, multiline); }
};

// ------------------------------------------------------------------ shapes compiled into this build
// (N, NV, MaxTerm, MaxLogLen, MaxMsgDomain)
#ifdef RMC_QUICK_BUILD
#define RMC_ORIG_SHAPES(X) X(3, 2, 3, 2, 5)
#else
#define RMC_ORIG_SHAPES(X) \
  X(3, 1, 2, 1, 2) /* C1 */ \
  X(3, 1, 2, 1, 6) /* safety_trio6: the smallest 3-server model with a commit */ \
  X(3, 2, 3, 2, 5) /* C2 */ \
  X(3, 2, 3, 2, 6)          \
  X(3, 2, 3, 2, 4)          \
  X(3, 2, 3, 2, 3)          \
  X(3, 2, 3, 2, 2)          \
  X(1, 2, 3, 2, 3)          \
  X(2, 1, 2, 1, 5)          \
  X(2, 1, 2, 1, 6)          \
  X(2, 1, 2, 1, 7) /* pair7: the smallest model in which commitIndex goes back */ \
  X(2, 1, 3, 2, 5)          \
  X(2, 2, 3, 2, 6)          \
  X(5, 1, 3, 3, 4) /* C5 */ \
  X(5, 2, 3, 3, 8) /* C5 with 2 values and 8 messages (compact election records) */ \
  X(5, 2, 2, 4, 6) /* 5 servers, one election term, 6 messages: compact election records within reach */
#endif

static Backend* orig_factory(const OrigModel& m) {
#define X(n, nv, mt, ml, mk) \
  if (m.N == n && m.NV == nv && m.MT == mt && m.ML == ml && m.MK == mk) return new OrigGpu<Orig<n, nv, mt, ml, mk>>(m);
  RMC_ORIG_SHAPES(X)
#undef X
  return nullptr;
}

static std::string compiled_shapes() {
  std::string o;
#define X(n, nv, mt, ml, mk) o += std::string(o.empty() ? "" : ", ") + "(" #n "," #nv "," #mt "," #ml "," #mk ")";
  RMC_ORIG_SHAPES(X)
#undef X
  return o;
}

Backend* make_orig_backend(const CfgFile& cfg) {
  OrigModel m = resolve_orig_model(cfg);
  Backend* b = orig_factory(m);
  if (!b) {
    std::ostringstream os;
    os << "raft_original shape (N=" << m.N << ", NV=" << m.NV << ", MaxTerm=" << m.MT << ", MaxLogLen=" << m.ML
       << ", MaxMsgDomain=" << m.MK << ") is not compiled into this build; compiled shapes (N,NV,MaxTerm,MaxLogLen,MaxMsgDomain): "
       << compiled_shapes();
    throw CfgError(MC_E_UNSUPPORTED, os.str());
  }
  return b;
}

}  // namespace rmc
