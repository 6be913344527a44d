// raftmc host: the framing of a checkpoint file (TLC -checkpoint / -recover),
// shared by the spec families and the generated path.  Host-only: no HIP header, so it compiles with
// a plain C++ compiler (tests/native/ckpt_file_check.cpp, tests/native/tlagen_ckpt_check.cpp).
//
// File: the backend's header (magic, the BFS position, TLC's counters), the text that names the model
// (a checkpoint only resumes the same model), the per-action generated and distinct counters,
// (states, generated) per level, then the stored states [0, total) in global-id order: fixed-width
// states and parent pointers (state_store.h), or the generated path's four arrays (GenHead).  The
// seen-set is rebuilt from the states on recovery.
#pragma once
#include <stdint.h>

#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/raftmc.h"

namespace rmc::ckpt {

// The on-disk headers, field order as written since their magics were introduced (the shared
// code below reads magic, nwp, n_act, n_levels and desc_len by name and copies the rest as bytes).
struct OrigHead {   // raft_original, "RAFTMCK2"
  char magic[8];
  uint64_t nwp, total, level_begin, level_count, seed;
  int64_t generated, distinct, depth, generated_in_model, n_act, n_levels, desc_len;
  // the search order the stored levels are in: 1 = TLC's single-worker FIFO order (-workers 1: kept
  // parents, per-action distinct counts and counterexamples are TLC's), 0 = the -workers N pipeline
  // (first-come dedup).  A -workers N checkpoint cannot resume a -workers 1 search (its kept
  // parents are not TLC's); the reverse is safe.
  int64_t fifo;
};
struct MembHead {   // tlc_membership, "RAFTMCM1"
  char magic[8];
  uint64_t nwp, total, level_begin, level_count, seed;
  uint64_t sym_tlc;   // the SYMMETRY mode the fingerprints were taken in (MC_COMPAT_SYM_TLC)
  int64_t generated, distinct, depth, generated_in_model, n_act, n_levels, desc_len;
};
// The generated path (csrc/tlagen), "RAFTMCG1": states are variable-width runs of canonical words,
// so nwp is 0 and the body is four arrays in global-id order, offs[total] (a state's first word),
// parent[total], act[total], words[words].  The writer lays the words out in id order: offs[0] = 0,
// offs ascends and state i ends where state i + 1 (or the array) begins.  fifo: as OrigHead's.
struct GenHead {
  char magic[8];
  uint64_t nwp, total, level_begin, level_count, seed;
  uint64_t words;     // canonical words stored
  int64_t fifo;
  int64_t generated, distinct, depth, generated_in_model, n_act, n_levels, desc_len;
};
static_assert(sizeof(OrigHead) == 112 && sizeof(MembHead) == 112, "the checkpoint headers are 112 bytes on disk");
static_assert(sizeof(GenHead) == 120, "the generated path's checkpoint header is 120 bytes on disk");

// a FILE* that is closed on every path (null when it could not be opened)
using File = std::unique_ptr<FILE, int (*)(FILE*)>;
inline File open_file(const std::string& path, const char* mode) { return File(std::fopen(path.c_str(), mode), std::fclose); }

// Writes `path`.tmp and renames it over `path` once everything is in it: a failed write never
// replaces (or creates) the checkpoint.  act_generated / act_distinct hold h.n_act counters each,
// levels h.n_levels elements with int64 members states and generated; body(FILE*) -> bool writes
// the stored states.
template <class H, class Levels, class Body>
int write_file(const std::string& path, const H& h, const std::string& desc, const std::vector<int64_t>& act_generated,
               const std::vector<int64_t>& act_distinct, const Levels& levels, Body body, std::string& err) {
  const std::string tmp = path + ".tmp";
  File f = open_file(tmp, "wb");
  if (!f) { err = "cannot write checkpoint " + tmp; return MC_E_IO; }
  const size_t na = (size_t)h.n_act;
  bool ok = std::fwrite(&h, sizeof h, 1, f.get()) == 1 && std::fwrite(desc.data(), 1, desc.size(), f.get()) == desc.size() &&
            std::fwrite(act_generated.data(), 8, na, f.get()) == na && std::fwrite(act_distinct.data(), 8, na, f.get()) == na;
  for (const auto& lv : levels) ok = ok && std::fwrite(&lv.states, 8, 1, f.get()) == 1 && std::fwrite(&lv.generated, 8, 1, f.get()) == 1;
  ok = ok && body(f.get());
  ok = std::fclose(f.release()) == 0 && ok;
  if (!ok || std::rename(tmp.c_str(), path.c_str()) != 0) { err = "writing checkpoint " + path + " failed"; return MC_E_IO; }
  return 0;
}

class Reader {
 public:
  explicit Reader(const std::string& path) : path_(path), f_(open_file(path, "rb")) {}
  FILE* file() const { return f_.get(); }
  // The header, the description and the counters.  A header of another family, model or state
  // width (or one cut short) is "not a checkpoint of this model"; counters cut short are "truncated".
  template <class H, class Levels>
  int head(const char* magic, uint64_t nwp, int64_t n_act, const std::string& desc, H& h, std::vector<int64_t>& act_generated,
           std::vector<int64_t>& act_distinct, Levels& levels, std::string& err) {
    if (!f_) { err = "cannot read checkpoint " + path_; return MC_E_IO; }
    std::string fdesc;
    bool ok = std::fread(&h, sizeof h, 1, f_.get()) == 1 && std::memcmp(h.magic, magic, 8) == 0 && h.nwp == nwp && h.n_act == n_act &&
              h.desc_len >= 0 && h.desc_len < (1 << 20) && h.n_levels > 0 && h.n_levels < (1 << 20);
    if (ok) { fdesc.resize((size_t)h.desc_len); ok = std::fread(&fdesc[0], 1, fdesc.size(), f_.get()) == fdesc.size(); }
    if (!ok || fdesc != desc) return other_model(err);
    const size_t na = (size_t)n_act;
    act_generated.resize(na); act_distinct.resize(na); levels.clear(); levels.resize((size_t)h.n_levels);
    ok = std::fread(act_generated.data(), 8, na, f_.get()) == na && std::fread(act_distinct.data(), 8, na, f_.get()) == na;
    for (auto& lv : levels) ok = ok && std::fread(&lv.states, 8, 1, f_.get()) == 1 && std::fread(&lv.generated, 8, 1, f_.get()) == 1;
    return ok ? 0 : truncated(err);
  }
  int other_model(std::string& err) const { err = "checkpoint " + path_ + " is not a checkpoint of this model"; return MC_E_INVALID; }
  int truncated(std::string& err) const { err = "checkpoint " + path_ + " is truncated"; return MC_E_IO; }

 private:
  std::string path_;
  File f_;
};

// The generated path's file behind Reader::head.  Every value a recovery later indexes with is
// checked on the host before anything is indexed: by check_gen_head the header's counts against
// each other, the levels and the file's length (so `total` and `words` are what the file holds);
// by read_gen_body offs against the writer's layout (GenHead) and a parent before its child
// (initial states, the first level, have none).  A file that fails is no checkpoint of this model.
template <class Levels>
int check_gen_head(Reader& in, const GenHead& h, const Levels& levels, std::string& err) {
  uint64_t in_levels = 0;
  for (const auto& lv : levels) {
    if (lv.states <= 0 || (uint64_t)lv.states > h.total) return in.other_model(err);
    in_levels += (uint64_t)lv.states;
  }
  if (h.total == 0 || h.total >= (1ull << 40) || h.words < h.total || h.words >= (1ull << 48) || in_levels != h.total ||
      h.level_count != (uint64_t)levels.back().states || h.level_begin != h.total - h.level_count ||
      h.depth != h.n_levels || h.distinct != (int64_t)h.total || (h.fifo != 0 && h.fifo != 1))
    return in.other_model(err);
  const long at = std::ftell(in.file());
  if (at < 0 || std::fseek(in.file(), 0, SEEK_END) != 0) return in.truncated(err);
  const long end = std::ftell(in.file());
  if (end < at || std::fseek(in.file(), at, SEEK_SET) != 0) return in.truncated(err);
  const uint64_t body = h.total * 20 + h.words * 4;
  if ((uint64_t)(end - at) < body) return in.truncated(err);
  if ((uint64_t)(end - at) > body) return in.other_model(err);
  return 0;
}
// The four arrays (after check_gen_head), read in chunks of at most chunk_bytes and handed to
// sink(kind, data, first, n, err) -> 0 or an error code: kind 0 offs, 1 parent, 2 act, 3 words;
// data[0] is element `first` of its array.  n_init: the initial states (the first level).
template <class Sink>
int read_gen_body(Reader& in, const GenHead& h, uint64_t n_init, size_t chunk_bytes, Sink sink, std::string& err) {
  const uint64_t most = h.total > (h.words + 1) / 2 ? h.total : (h.words + 1) / 2;   // the longest array, in 8-byte units
  std::vector<uint64_t> buf(chunk_bytes / 8 == 0 ? 1 : chunk_bytes / 8 < most ? chunk_bytes / 8 : most);
  uint64_t prev_off = 0;
  for (int kind = 0; kind < 4; ++kind) {
    const size_t esz = kind < 2 ? 8 : 4;
    const uint64_t len = kind == 3 ? h.words : h.total, per = buf.size() * 8 / esz;
    for (uint64_t first = 0; first < len; first += per) {
      const uint64_t n = len - first < per ? len - first : per;
      if (std::fread(buf.data(), esz, n, in.file()) != n) return in.truncated(err);
      for (uint64_t k = 0; kind == 0 && k < n; ++k) {
        const uint64_t o = buf[k];
        if (first + k == 0 ? o != 0 : (o <= prev_off || o >= h.words)) return in.other_model(err);
        prev_off = o;
      }
      for (uint64_t k = 0; kind == 1 && k < n; ++k)
        if (first + k < n_init ? buf[k] != ~0ull : buf[k] >= first + k) return in.other_model(err);
      if (int rc = sink(kind, (const void*)buf.data(), first, n, err)) return rc;
    }
  }
  return 0;
}

// ---------------------------------------------------------------- multi-GPU checkpoints
// A raft_original search on W > 1 GPUs writes, every time it checkpoints, one file per rank,
// `path`.g<G>.r<k> (G, the generation: the levels completed), and then the manifest `path`.  Both
// have the framing above around one header:
//  - the manifest ("RAFTMCS1", rank -1, no body): the search's counters, total = distinct, the
//    per-action counters and the (states, generated) of every level;
//  - a rank file ("RAFTMCR1"): the same counters, total / level_begin / level_count of that rank's
//    store, its level rows (states = the rank's states of the level, generated = the level's states
//    over all ranks, which must be the manifest's), then the rank's stored states and their parent
//    pointers (rank-tagged ids) as a single-GPU file holds them.
struct ShardHead {
  char magic[8];
  uint64_t nwp, total, level_begin, level_count, seed;
  int64_t generated, distinct, depth, generated_in_model, n_act, n_levels, desc_len;
  int64_t fifo;                       // 0: the sharded search is a -workers N search
  int64_t rank, world, generation;
};
static_assert(sizeof(ShardHead) == 136, "the multi-GPU checkpoint headers are 136 bytes on disk");
constexpr const char* kManifestMagic = "RAFTMCS1";
constexpr const char* kRankMagic = "RAFTMCR1";
constexpr const char* kOrigMagic = "RAFTMCK2";

struct LevelRow { int64_t states = 0, generated = 0; };

inline std::string rank_path(const std::string& path, int64_t generation, int rank) {
  return path + ".g" + std::to_string(generation) + ".r" + std::to_string(rank);
}

// the first 8 bytes of `path` ("" when it has fewer or cannot be read)
inline std::string file_magic(const std::string& path) {
  const File f = open_file(path, "rb");
  char m[8];
  return f && std::fread(m, 1, 8, f.get()) == 8 ? std::string(m, 8) : std::string();
}

// the rank files of the manifest at `path` (if it is one) that a manifest of `generation` and
// `world` does not name: what the writer removes once the new manifest is in place
inline void remove_stale_rank_files(const std::string& path, int64_t old_generation, int64_t old_world, int64_t generation, int64_t world) {
  for (int64_t k = 0; k < old_world && k < 8; ++k)
    if (old_generation != generation || k >= world) (void)std::remove(rank_path(path, old_generation, (int)k).c_str());
}

// What a recovery reads (orig_reshard.hip): W parts, each a file that holds, from `body` on, the
// `total` states of one source rank and then their parent pointers, level after level
// (level_count[L] of them in level L).  A single-GPU file is one part with untagged ids.
struct SourcePart {
  std::string path;
  uint64_t body = 0, total = 0;
  std::vector<uint64_t> level_count;
};
struct ShardSource {
  int world = 0;
  bool sharded = false;               // a manifest (ids carry their rank) / a single-GPU file
  uint64_t seed = 0;
  int64_t fifo = 0, generated = 0, distinct = 0, depth = 0, generated_in_model = 0, generation = 0;
  std::vector<int64_t> act_generated, act_distinct;
  std::vector<LevelRow> levels;       // of the whole search
  std::vector<SourcePart> parts;
};

// the bytes behind the read position, which stays where it was
inline bool bytes_left(FILE* f, uint64_t& n) {
  const long at = std::ftell(f);
  if (at < 0 || std::fseek(f, 0, SEEK_END) != 0) return false;
  const long end = std::ftell(f);
  if (end < at || std::fseek(f, at, SEEK_SET) != 0) return false;
  n = (uint64_t)(end - at);
  return true;
}

// Opens the source at `path` for a model of nwp words, n_act actions and description desc: a
// manifest with its rank files, or a single-GPU raft_original file.  Everything a recovery later
// indexes with is checked here, on the host: the level tables against the totals, the rank files
// against the manifest (generation, world, rank, seed, levels) and each file's length.  A missing rank
// file, one of another generation, world, rank or model, and tables that disagree are
// MC_E_INVALID; a file shorter than its header says is MC_E_IO.
inline int open_source(const std::string& path, uint64_t nwp, int64_t n_act, const std::string& desc, ShardSource& s, std::string& err) {
  s = ShardSource();
  const uint64_t slot = nwp * 4 + 8;
  const std::string magic = file_magic(path);
  if (magic != kManifestMagic) {   // a single-GPU file (or nothing Reader::head accepts)
    OrigHead h;
    Reader in(path);
    if (int rc = in.head(kOrigMagic, nwp, n_act, desc, h, s.act_generated, s.act_distinct, s.levels, err)) return rc;
    uint64_t in_levels = 0, left = 0;
    SourcePart p;
    for (const auto& lv : s.levels) {
      if (lv.states <= 0 || (uint64_t)lv.states > h.total) return in.other_model(err);
      in_levels += (uint64_t)lv.states;
      p.level_count.push_back((uint64_t)lv.states);
    }
    if (h.total == 0 || h.total > (1ull << 37) || in_levels != h.total || h.level_count != (uint64_t)s.levels.back().states ||
        h.level_begin != h.total - h.level_count || h.depth != h.n_levels || h.distinct != (int64_t)h.total || (h.fifo != 0 && h.fifo != 1))
      return in.other_model(err);
    if (!bytes_left(in.file(), left) || left < h.total * slot) return in.truncated(err);
    if (left > h.total * slot) return in.other_model(err);
    p.path = path; p.body = (uint64_t)std::ftell(in.file()); p.total = h.total;
    s.parts.push_back(p);
    s.world = 1; s.sharded = false; s.seed = h.seed; s.fifo = h.fifo; s.generated = h.generated; s.distinct = h.distinct;
    s.depth = h.depth; s.generated_in_model = h.generated_in_model; s.generation = h.depth;
    return 0;
  }
  ShardHead m;
  {
    Reader in(path);
    if (int rc = in.head(kManifestMagic, nwp, n_act, desc, m, s.act_generated, s.act_distinct, s.levels, err)) return rc;
    uint64_t in_levels = 0, left = 0;
    for (const auto& lv : s.levels) {
      if (lv.states <= 0 || (uint64_t)lv.states > m.total) return in.other_model(err);
      in_levels += (uint64_t)lv.states;
    }
    if (m.world < 1 || m.world > 8 || m.rank != -1 || m.fifo != 0 || m.total == 0 || m.total >= (1ull << 40) || in_levels != m.total ||
        m.level_count != (uint64_t)s.levels.back().states || m.level_begin != m.total - m.level_count || m.depth != m.n_levels ||
        m.generation != m.depth || m.distinct != (int64_t)m.total)
      return in.other_model(err);
    if (!bytes_left(in.file(), left)) return in.truncated(err);
    if (left != 0) return in.other_model(err);
  }
  std::vector<uint64_t> level_sum(s.levels.size(), 0);
  for (int k = 0; k < (int)m.world; ++k) {
    SourcePart p;
    p.path = rank_path(path, m.generation, k);
    Reader in(p.path);
    if (!in.file()) { err = "checkpoint " + path + ": rank file " + p.path + " is missing"; return MC_E_INVALID; }
    ShardHead h;
    std::vector<int64_t> ag, ad;
    std::vector<LevelRow> rows;
    if (int rc = in.head(kRankMagic, nwp, n_act, desc, h, ag, ad, rows, err)) return rc;
    if (h.rank != k || h.world != m.world || h.generation != m.generation || h.seed != m.seed || h.n_levels != m.n_levels ||
        h.total > (1ull << 37))
      return in.other_model(err);
    uint64_t mine = 0, left = 0;
    for (size_t l = 0; l < rows.size(); ++l) {
      if (rows[l].generated != s.levels[l].states || rows[l].states < 0 || rows[l].states > s.levels[l].states) return in.other_model(err);
      mine += (uint64_t)rows[l].states;
      level_sum[l] += (uint64_t)rows[l].states;
      p.level_count.push_back((uint64_t)rows[l].states);
    }
    if (mine != h.total || h.level_count != p.level_count.back() || h.level_begin != h.total - h.level_count) return in.other_model(err);
    if (!bytes_left(in.file(), left) || left < h.total * slot) return in.truncated(err);
    if (left > h.total * slot) return in.other_model(err);
    p.body = (uint64_t)std::ftell(in.file()); p.total = h.total;
    s.parts.push_back(p);
  }
  for (size_t l = 0; l < s.levels.size(); ++l)
    if (level_sum[l] != (uint64_t)s.levels[l].states) {
      err = "checkpoint " + path + ": the rank files' level tables disagree with the manifest";
      return MC_E_INVALID;
    }
  s.world = (int)m.world; s.sharded = true; s.seed = m.seed; s.fifo = 0; s.generated = m.generated; s.distinct = m.distinct;
  s.depth = m.depth; s.generated_in_model = m.generated_in_model; s.generation = m.generation;
  return 0;
}

}  // namespace rmc::ckpt
