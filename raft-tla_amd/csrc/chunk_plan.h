// raftmc — how one BFS level of the single-GPU -workers N search is cut into chunks (host only).
//
// The record buffers of a chunk (orig_backend.hip: d_rfp_, d_rkey_, d_rcnt_blk_, d_lead_) are two
// halves of one allocation.  A level below the threshold, or any level when the sub-chunk size is 0,
// runs in chunks of the whole allocation on one stream (buffer 0 from its start).  A larger level is
// cut into sub-chunks that alternate between the two halves, so orig_generate of sub-chunk c + 1 can
// run beside the seen-set probes of sub-chunk c.  Every chunk but a level's last is a whole number
// of workgroups: records are grouped per generate workgroup.  A level whose first parents were generated
// ahead, beside the level before's last dedup (the level hoist), starts with that prefix
// as its chunk 0, in the half it was generated into.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <vector>

namespace rmc {

// Defaults of the pipelined schedule, measured on C2 (DESIGN.md §0e,
// profiles/r08_generate_dedup_overlap_ab.txt).  Sub-chunks as large as a half holds: smaller ones lose
// to the single stream or gain nothing (256K +9 ms, 512K +6, 1M +0.6, 1.65M -0.2, 2M -0.5, a half of
// 2.47M -1.0 ms per C2 run), so a half that holds fewer than OVERLAP_MIN_HALF parents is never used.
// Smallest level that is split: 0, 3M and 5M were within the run-to-run spread of each other; 4M
// leaves the levels that gain nothing on one stream.
constexpr uint64_t OVERLAP_STATES = 1ull << 24;       // orig_scan's chunk limit: always cut to the half
constexpr uint64_t OVERLAP_MIN_HALF = 2ull << 20;
constexpr uint64_t OVERLAP_MIN_LEVEL = 4ull << 20;

struct Chunk {
  uint64_t first, count;   // the chunk's parents: level index of the first one, how many
  int buffer;              // 0 / 1: which half of the record buffers
};

struct ChunkPlan {
  uint64_t half_cap = 0;   // parents one half holds, whole workgroups (the second half is no smaller)
  uint64_t full_cap = 0;   // parents the whole allocation holds, whole workgroups
  uint64_t sub = 0;        // sub-chunk size; 0 = never split
  uint64_t threshold = 0;  // levels with fewer parents are not split
  int wg = 256;            // workgroup size

  static uint64_t round_wg(uint64_t v, uint64_t wg) { return (v + wg - 1) / wg * wg; }

  // full: parents the whole allocation holds (a multiple of wg).  sub_states is rounded up to whole
  // workgroups, at least one workgroup and at most one half.
  ChunkPlan(uint64_t full, uint64_t sub_states, uint64_t min_level, int wg_size = 256) : wg(wg_size) {
    const uint64_t w = (uint64_t)wg;
    full_cap = full / w * w;
    half_cap = full_cap / 2 / w * w;
    if (sub_states && half_cap) {
      sub = round_wg(sub_states, w);
      if (sub > half_cap) sub = half_cap;
    }
    threshold = min_level;
  }

  // the default sub-chunk size for an allocation of full parents (0: the halves are too small)
  static uint64_t default_sub(uint64_t full, uint64_t wg_size = 256) {
    return full / 2 / wg_size * wg_size >= OVERLAP_MIN_HALF ? OVERLAP_STATES : 0;
  }

  bool split(uint64_t level_count) const { return sub != 0 && level_count >= threshold && level_count > sub; }

  // whether a level's first pre_count parents can have been generated ahead into one half (the level
  // hoist): whole workgroups unless they are the whole level, and no more than a half
  bool prefix_ok(uint64_t level_count, uint64_t pre_count) const {
    return sub != 0 && pre_count <= level_count && pre_count <= half_cap &&
           (pre_count % (uint64_t)wg == 0 || pre_count == level_count);
  }

  // the chunks of a level, in order; returns whether the level is split (pipelined).
  // pre_count > 0: the level's first pre_count parents were generated ahead into half pre_buffer.  They
  // are chunk 0 as they stand, the rest follows in sub-chunks from the other half on, and the level is
  // pipelined whatever its size (an unsplit chunk would write over the prefix's records).  A prefix
  // that is not prefix_ok() gives no plan: out is left empty.
  bool plan(uint64_t level_count, std::vector<Chunk>& out, uint64_t pre_count = 0, int pre_buffer = 0) const {
    out.clear();
    if (pre_count) {
      if (!prefix_ok(level_count, pre_count)) return false;
      int b = pre_buffer & 1;
      out.push_back({0, pre_count, b});
      for (uint64_t first = pre_count; first < level_count; first += sub) {
        const uint64_t left = level_count - first;
        out.push_back({first, left < sub ? left : sub, b ^= 1});
      }
      return true;
    }
    const bool sp = split(level_count);
    const uint64_t step = sp ? sub : full_cap;
    int b = 0;
    for (uint64_t first = 0; first < level_count; first += step) {
      const uint64_t left = level_count - first;
      out.push_back({first, left < step ? left : step, sp ? b : 0});
      b ^= 1;
    }
    return sp;
  }
};

// RAFTMC_OVERLAP_STATES-style variable: a whole non-negative number, or the default
inline uint64_t env_u64(const char* name, uint64_t dflt) {
  const char* s = std::getenv(name);
  if (!s || !*s) return dflt;
  char* end = nullptr;
  const unsigned long long v = std::strtoull(s, &end, 0);
  return (end != s && *end == 0) ? (uint64_t)v : dflt;
}

}  // namespace rmc
