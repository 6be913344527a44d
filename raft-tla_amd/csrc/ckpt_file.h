// raftmc host: the framing of a checkpoint file (TLC -checkpoint / -recover),
// shared by the spec families.  Host-only: no HIP header, so it compiles with a plain C++ compiler
// (tests/native/ckpt_file_check.cpp).
//
// File: the family's 112-byte header (magic, the BFS position, TLC's counters), the model's
// describe_json text (a checkpoint only resumes the same model), the per-action generated and
// distinct counters, (states, generated) per level, then the stored states and parent pointers
// [0, total) in global-id order (state_store.h).  The seen-set is rebuilt from the states on recovery.
#pragma once
#include <stdint.h>

#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/raftmc.h"

namespace rmc::ckpt {

// The two on-disk headers, field order as written since their magics were introduced (the shared
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
static_assert(sizeof(OrigHead) == 112 && sizeof(MembHead) == 112, "the checkpoint headers are 112 bytes on disk");

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

}  // namespace rmc::ckpt
