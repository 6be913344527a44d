// TEST HARNESS ONLY (never part of the product).  Continue mode on the host: a
// single-worker FIFO BFS with the product's packed tlc_membership spec (raft-tla_amd/csrc/memb_spec.h,
// the header the gfx950 kernels compile), modelled on memb_host_bfs.cpp.  The search runs as for a cfg
// without invariants; every checked successor (new, or out of the model unless INV_OOM=0) is evaluated
// against each listed invariant that has no witness yet, S::inv per cfg position.  Walking the
// successors in TLC's enumeration order, the first violating one per invariant is its witness (the
// minimum key of the first level that has any); an invariant that fails to evaluate ends the run.
// Shape: -DSHAPE_N=.. -DSHAPE_NV=..
//   memb_witness_host CFG MAX_DEPTH
//     -> one JSON line per witness {invariant, position, depth, key, generated, distinct, left_on_queue,
//        state}, then {"summary": ...}
// SYM_TLC=1 (environment): TLC-mode symmetry, as MC_COMPAT_SYM_TLC.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <unordered_set>
#include <vector>

#include "../../raft-tla_amd/csrc/memb_text.h"

using namespace rmc;
using S = Memb<SHAPE_N, SHAPE_NV, 2 * SHAPE_N * SHAPE_N>;
using W = S::Work;

static std::string json_escape(const std::string& x) {
  std::string o;
  for (char ch : x) { if (ch == '"' || ch == '\\') o += '\\'; o += ch; }
  return o;
}

int main(int argc, char** argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: memb_witness_host CFG MAX_DEPTH\n"); return 2; }
  CfgFile cfg = parse_cfg_text(read_text_file(argv[1]));
  MembModel m = resolve_memb_model(cfg);
  const long long max_depth = std::atoll(argv[2]);
  MembText<S> text(m);
  MembRuntime rt = m.rt;
  if (std::getenv("SYM_TLC") && rt.symmetry) rt.sym_tlc = 1;
  const char* oomenv = std::getenv("INV_OOM");
  const bool inv_oom = !(oomenv && std::string(oomenv) == "0");
  auto inv_id = [&](u32 q) { return (int)((rt.inv_order[q / 8] >> (8 * (q % 8))) & 255u); };
  const u64 seed = 0x5EED5EED2024ull;
  std::unordered_set<u64> seen;
  std::vector<W> frontier(1);
  S::init(frontier[0]);
  seen.insert(S::fingerprint(frontier[0], seed, rt));
  long long generated = 1, left = 0, nwit = 0;
  int depth = 1;
  u32 err = 0, pending = rt.n_inv >= 32 ? ~0u : (1u << rt.n_inv) - 1u;
  std::string verdict = "OK";
  // the pending invariants on one checked state; a witness is printed with the counters of its stop point
  auto check = [&](const W& t, int wdepth, long long key, long long wleft) {
    for (u32 q = 0; q < rt.n_inv; ++q) {
      if (!((pending >> q) & 1u)) continue;
      const int r = S::inv(t, inv_id(q), rt);
      if (r == IV_ERR) { verdict = "EVAL_ERROR"; return; }
      if (r != IV_BAD) continue;
      std::printf("{\"invariant\": \"%s\", \"position\": %u, \"depth\": %d, \"key\": %lld, \"generated\": %lld, \"distinct\": %zu, "
                  "\"left_on_queue\": %lld, \"state\": \"%s\"}\n",
                  kMembInvNames[inv_id(q)], q, wdepth, key, generated, seen.size(), wleft, json_escape(text.text(t, false)).c_str());
      pending &= ~(1u << q);
      ++nwit;
    }
  };
  check(frontier[0], 1, 0, 0);
  bool done = verdict != "OK" || (nwit && !pending);
  while (!frontier.empty() && !done) {
    if (max_depth && depth >= max_depth) { left = (long long)frontier.size(); break; }
    std::vector<W> next;
    for (size_t fi = 0; fi < frontier.size() && !done; ++fi) {
      const W& s = frontier[fi];
      // TLC (oracle) counts a state's whole successor list before checking any of them
      for (int k = 0; k < S::NI; ++k) {
        if (!S::group_enabled(k, rt.next)) continue;
        for (int sub = 0; sub < S::nsub(k); ++sub) { W t; if (S::apply(s, k, sub, t, err, rt) >= 0) generated += S::tlc_copies(s, k, sub, rt); }
      }
      for (int k = 0; k < S::NI && !done; ++k) {
        if (!S::group_enabled(k, rt.next)) continue;
        for (int sub = 0; sub < S::nsub(k) && !done; ++sub) {
          W t;
          if (S::apply(s, k, sub, t, err, rt) < 0) continue;
          const bool im = S::in_model(t, s, rt);
          bool isnew = false;
          if (im) {
            isnew = seen.insert(S::fingerprint(t, seed, rt)).second;
            if (isnew) next.push_back(t);
          }
          if (isnew || (!im && inv_oom)) {
            check(t, depth + 1, (long long)fi * S::NSLOT + S::slot_of(k, sub), (long long)(frontier.size() - fi - 1 + next.size()));
            done = verdict != "OK" || (nwit && !pending);
            if (done) left = (long long)(frontier.size() - fi - 1 + next.size());
          }
        }
      }
    }
    if (done) { depth++; break; }
    if (!next.empty()) depth++;
    frontier.swap(next);
  }
  std::printf("{\"summary\": {\"generated\": %lld, \"distinct\": %zu, \"depth\": %d, \"left_on_queue\": %lld, \"err\": %u, "
              "\"verdict\": \"%s\", \"witnesses\": %lld, \"pending\": %u}}\n",
              generated, seen.size(), depth, left, err, verdict.c_str(), nwit, pending);
  return 0;
}
