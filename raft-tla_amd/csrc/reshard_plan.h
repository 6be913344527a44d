// raftmc — the index arithmetic of recovering a raft_original checkpoint at another GPU count
// (DESIGN.md §3f), shared by the kernels of orig_reshard.hip and the host (tests/native/
// reshard_plan_check.cpp compiles it without HIP).
//
// A stored state's global id is owner rank << 37 | index in the owner's store; a single-GPU file is
// world 1 with rank 0.  Every rank stores its levels one behind the other, so level L of a source
// of W ranks is W slices.  The canonical order of a level is rank 0's slice, then rank 1's, ...:
// the order in which every target rank reads it, so every target rank computes the same new ids.
#pragma once
#include "common.h"

namespace rmc {

constexpr int RESHARD_MAX_WORLD = 8;
constexpr int GID_RANK_SHIFT = 37;                        // a global id: rank << 37 | local index
constexpr u64 GID_LOCAL_MASK = (1ull << GID_RANK_SHIFT) - 1;
constexpr int META_GID_SHIFT = 24;                        // a parent pointer: parent id << 24 | action << 16 | low bits

// one level of the source as its ranks hold it
struct ReshardLevel {
  u64 begin[RESHARD_MAX_WORLD];   // index in rank r's store of its first state of the level
  u64 count[RESHARD_MAX_WORLD];   // rank r's states of the level
  u64 off[RESHARD_MAX_WORLD];     // canonical position of rank r's first state in the level
  u32 world;                      // 0: no level (the parents of the initial states)
};

// fills off[] from count[]; returns the level's size
RMC_HD u64 reshard_canonical(ReshardLevel& lv) {
  u64 at = 0;
  for (u32 r = 0; r < (u32)RESHARD_MAX_WORLD; ++r) {
    lv.off[r] = at;
    if (r < lv.world) at += lv.count[r];
  }
  return at;
}

// the canonical position in `lv` of the state with the source id `old_id`; false when the id
// does not name a state of that level (nothing is indexed with a value that fails here)
RMC_HD bool reshard_position(const ReshardLevel& lv, u64 old_id, u64& pos) {
  const u64 rank = old_id >> GID_RANK_SHIFT, local = old_id & GID_LOCAL_MASK;
  bool found = false;
  for (u32 r = 0; r < (u32)RESHARD_MAX_WORLD; ++r) {   // (a select per rank: no indexing by a value of the file)
    if (r >= lv.world || (u64)r != rank) continue;
    if (local >= lv.begin[r] && local - lv.begin[r] < lv.count[r]) { pos = lv.off[r] + (local - lv.begin[r]); found = true; }
  }
  return found;
}

// the new id of the idx-th state (canonical order) of a level among those `owner` receives;
// owner_level_begin: the states the owner received from the levels before
RMC_HD u64 reshard_new_id(u32 owner, u64 owner_level_begin, u64 idx) {
  return ((u64)owner << GID_RANK_SHIFT) | (owner_level_begin + idx);
}

// a parent pointer with its parent id replaced: the action byte and the low bits stay
RMC_HD u64 reshard_meta(u64 meta, u64 new_parent) {
  return (meta & ((1ull << META_GID_SHIFT) - 1)) | (new_parent << META_GID_SHIFT);
}

}  // namespace rmc
