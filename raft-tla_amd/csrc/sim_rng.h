// raftmc — simulation mode (TLC -simulate): the counter-based random numbers and the successor
// selection rule, shared by the gfx950 walker (orig_sim.hip), the host replay of one walk and the
// test mirror (tests/native/orig_sim_host.cpp).
//
// Every draw is a pure function of (seed, walk, step, draw index): a walk is reproducible on its
// own, and nothing depends on the grid shape, on timing or on the order of atomics.  TLC's own
// RNG stream is not reproduced.
//
// Selection (reservoir sampling, size 1): a step's in-model successors are numbered j = 1, 2, ..
// in apply's instance order; candidate j replaces the one kept so far iff sim_pick(draw j, j) == 0,
// i.e. with probability ~1/j (j = 1: always), so each of n candidates ends up kept with
// probability ~1/n.  sim_pick maps a 32-bit draw onto [0, n) by a multiply and a shift: the bias
// is below n / 2^32 (n <= 255 instances).
#pragma once
#include "common.h"

namespace rmc {

constexpr int64_t SIM_DEFAULT_DEPTH = 100;       // TLC's -depth default in simulation mode
constexpr int64_t SIM_DEFAULT_BATCH = 262144;    // walkers per launch (a constant, not a device query)
constexpr int64_t SIM_MAX_DEPTH = 16383;         // the event word holds the trace length in 14 bits
constexpr int64_t SIM_MAX_WALKS = 1ll << 40;     // ... and the walk number in 40

// the key of (seed, walk, step): two rounds of fmix64, once per step
RMC_HD u64 sim_step_key(u64 seed, u64 walk, u32 step) {
  u64 h = fmix64(seed ^ (walk + 1) * P1);
  return fmix64(h ^ ((u64)step + 1) * P5);
}
// draw `idx` of a step: 32 bits (murmur3's 32-bit finaliser over the key's halves and the index)
RMC_HD u32 sim_draw(u64 key, u32 idx) {
  u32 x = (u32)key ^ (idx * 0x9E3779B1u);
  x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
  x += (u32)(key >> 32);
  x ^= x >> 15; x *= 0x2C1B3C6Du; x ^= x >> 12;
  return x;
}
// a 32-bit draw onto [0, n)
RMC_HD u32 sim_pick(u32 r32, u32 n) { return (u32)(((u64)r32 * (u64)n) >> 32); }
// reservoir rule: does in-model candidate j (1-based, instance order) replace the one kept so far?
RMC_HD bool sim_take(u64 key, u32 j) { return sim_pick(sim_draw(key, j), j) == 0u; }

// 64-bit event word of a batch, minimum wins: (trace length, walk, instance, kind); the kinds are
// the BFS's (EV_NEXT_ERROR .. EV_VIOLATION).  Trace length = states up to and including the one the
// event is about (the violating successor; the state whose successors raised the error; the
// deadlocked state).
RMC_HD u64 sim_event(u64 length, u64 walk, u32 inst, u32 kind) { return (((length << 40 | walk) << 8 | (u64)inst) << 2) | (u64)kind; }
RMC_HD u64 sim_event_length(u64 e) { return e >> 50; }
RMC_HD u64 sim_event_walk(u64 e) { return (e >> 10) & lomask(40); }
RMC_HD u32 sim_event_inst(u64 e) { return (u32)(e >> 2) & 255u; }
RMC_HD u32 sim_event_kind(u64 e) { return (u32)e & 3u; }

}  // namespace rmc
