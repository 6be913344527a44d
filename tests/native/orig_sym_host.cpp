// TEST HARNESS ONLY (never part of the product).  SYMMETRY Permutations(Server) for raft_original
// on the host, over the header the gfx950 kernels compile (raft-tla_amd/csrc/orig_spec.h):
//
//   orig_sym_host CFG [--seed S] [--max-depth D]
//       a single-worker FIFO BFS whose seen-set holds one S::fp_sym fingerprint per orbit: the
//       kept, expanded and counted state is the successor as generated (never a normalised copy),
//       "generated" counts the successors of kept states, "distinct" counts orbits.  One JSON
//       line: verdict, violated, generated, distinct, depth, levels, actions {name: [generated,
//       distinct]}, trace_len.
//   orig_sym_host CFG --check [--seed S]
//       every state of the UNSYMMETRIC BFS of the cfg (full packed states in the seen-set) ...
//   orig_sym_host CFG --check-walks NUM DEPTH [--seed S]
//       ... or the distinct states along NUM seeded random walks of DEPTH states (the simulation
//       mode's draws, sim_rng.h); the even walks start at Init, the odd ones behind a scripted first
//       election (first_election below: uniform walks of a 5-server model practically never hold
//       one, and the election records are what the compact layout is about), checked against
//       S::permute for all N! permutations p:
//         fp_sym(permute(s, p)) == fp_sym(s);  permute by p, then by p's inverse, is s;
//         permute(s, p) is canonical (sorted sets) and survives pack / unpack;
//         the partition by fp_sym equals the partition by the least packed image over all p;
//         the sum over orbits of N! / |stabiliser| (= the states when the set is closed).
//       One JSON line: states, with_elections (states whose elections set is not empty), orbits, orbit_sum, disagreements, bad_fp, bad_inverse, bad_pack.
// Shape: -DSHAPE_N=.. -DSHAPE_NV=.. -DSHAPE_MT=.. -DSHAPE_ML=.. -DSHAPE_MK=..
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <unordered_set>
#include <vector>

#include "../../raft-tla_amd/csrc/orig_text.h"
#include "../../raft-tla_amd/csrc/sim_rng.h"

using namespace rmc;
using S = Orig<SHAPE_N, SHAPE_NV, SHAPE_MT, SHAPE_ML, SHAPE_MK>;
using W = S::Work;
using Words = std::vector<u32>;

static Words packed(const W& s) { u32 a[S::NW]; S::pack(s, a); return Words(a, a + S::NW); }

static bool same_work(const W& a, const W& b) {
  bool ok = a.term == b.term && a.st == b.st && a.voted == b.voted && a.commit == b.commit && a.vresp == b.vresp && a.vgrant == b.vgrant;
  for (int i = 0; i < S::N; ++i)
    ok = ok && a.nexti.v[i] == b.nexti.v[i] && a.matchi.v[i] == b.matchi.v[i] && a.log.v[i] == b.log.v[i] && a.vl.v[i] == b.vl.v[i];
  for (int k = 0; k < S::AW; ++k) ok = ok && a.allLogs[k] == b.allLogs[k];
  for (int k = 0; k < S::EMAX; ++k) ok = ok && a.el[k] == b.el[k];
  for (int k = 0; k < S::MK + 1; ++k) ok = ok && a.bag.v[k] == b.bag.v[k];
  return ok;
}

// sets strictly ascending with the empty slots last: the canonical working form
static bool canonical(const W& t) {
  for (int k = 0; k + 1 < S::EMAX; ++k) if (t.el[k] != S::EMPTY || t.el[k + 1] != S::EMPTY) if (!(t.el[k] < t.el[k + 1])) return false;
  for (int k = 0; k + 1 < S::MK + 1; ++k)
    if (t.bag.v[k] != S::BEMPTY || t.bag.v[k + 1] != S::BEMPTY) if (!(t.bag.v[k] < t.bag.v[k + 1])) return false;
  return true;
}

struct Check {
  u64 seed = 1;
  long long states = 0, with_elections = 0, orbits = 0, orbit_sum = 0, disagreements = 0, bad_fp = 0, bad_inverse = 0, bad_pack = 0;
  std::map<u64, Words> by_fp;
  std::map<Words, u64> by_canon;
  void state(const W& s) {
    ++states;
    if (s.el[0] != S::EMPTY) ++with_elections;
    const u64 f = S::fp_sym(s, seed);
    if (f == 0) ++bad_fp;
    const Words p0 = packed(s);
    Words canon = p0;
    long long stab = 0;
    for (int p = 0; p < S::NPERM; ++p) {
      const u32 pi = S::perm_of(p);
      W t, back, u;
      S::permute(s, pi, t);
      if (S::fp_sym(t, seed) != f) ++bad_fp;
      S::permute(t, S::perm_inverse(pi), back);
      if (!same_work(back, s)) ++bad_inverse;
      const Words pt = packed(t);
      u32 a[S::NW];
      for (int q = 0; q < S::NW; ++q) a[q] = pt[q];
      S::unpack(a, u);
      if (!canonical(t) || !same_work(u, t)) ++bad_pack;
      if (pt == p0) ++stab;
      if (pt < canon) canon = pt;
    }
    auto a = by_fp.find(f);
    if (a != by_fp.end() && a->second != canon) ++disagreements;    // one fingerprint, two orbits
    auto b = by_canon.find(canon);
    if (b != by_canon.end() && b->second != f) ++disagreements;     // one orbit, two fingerprints
    if (b == by_canon.end()) { ++orbits; orbit_sum += S::NPERM / stab; by_canon.emplace(canon, f); }
    if (a == by_fp.end()) by_fp.emplace(f, canon);
  }
  void print() const {
    std::printf("{\"states\": %lld, \"with_elections\": %lld, \"orbits\": %lld, \"orbit_sum\": %lld, \"permutations\": %d, \"disagreements\": %lld, "
                "\"bad_fp\": %lld, \"bad_inverse\": %lld, \"bad_pack\": %lld}\n",
                states, with_elections, orbits, orbit_sum, S::NPERM, disagreements, bad_fp, bad_inverse, bad_pack);
  }
};

// The state after the shortest first election: Timeout(s1), then for each voter RequestVote, (UpdateTerm,)
// HandleRequestVoteRequest, HandleRequestVoteResponse, until BecomeLeader is enabled -- at every step
// the first in-model successor of the most advanced action.  false: no election within 64 steps.
static bool first_election(const OrigModel& m, W& out) {
  static const int prio[] = {OA_BecomeLeader, OA_HandleRequestVoteResponse, OA_HandleRequestVoteRequest, OA_UpdateTerm, OA_RequestVote, OA_Timeout};
  W cur; S::init(cur);
  for (int step = 0; step < 64; ++step) {
    bool moved = false;
    for (int want : prio) {
      if (want == OA_Timeout && cur.st != 0) continue;   // one candidate only
      for (int k = 0; k < S::NI && !moved; ++k) {
        W t; u32 err = 0;
        if (S::apply(cur, k, t, err) != want) continue;
        S::all_logs_next(cur, t.allLogs);
        if (!S::in_model(t, m.rt)) continue;
        cur = t; moved = true;
        if (want == OA_BecomeLeader) { out = cur; return true; }
      }
      if (moved) break;
    }
    if (!moved) return false;
  }
  return false;
}

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: orig_sym_host CFG [--seed S] [--max-depth D] [--check | --check-walks NUM DEPTH]\n"); return 2; }
  CfgFile cfg = parse_cfg_text(read_text_file(argv[1]));
  if (!cfg.symmetry.empty()) cfg.symmetry_def = "Permutations(Server)";   // the harness takes the name on trust
  const OrigModel m = resolve_orig_model(cfg);
  u64 seed = 1;
  long long max_depth = 0, walks = 0, walk_depth = 0;
  bool check = false;
  for (int a = 2; a < argc; ++a) {
    const std::string k = argv[a];
    if (k == "--seed" && a + 1 < argc) seed = std::strtoull(argv[++a], nullptr, 0);
    else if (k == "--max-depth" && a + 1 < argc) max_depth = std::atoll(argv[++a]);
    else if (k == "--check") check = true;
    else if (k == "--check-walks" && a + 2 < argc) { walks = std::atoll(argv[++a]); walk_depth = std::atoll(argv[++a]); }
    else { std::fprintf(stderr, "unknown argument %s\n", argv[a]); return 2; }
  }
  W s0; S::init(s0);

  if (walks > 0) {   // the states along seeded walks (orig_sim_host.cpp's rule), each distinct one checked once
    Check c; c.seed = seed;
    std::set<Words> done;
    W elected;
    if (!first_election(m, elected)) { std::printf("{\"error\": \"no first election\"}\n"); return 1; }
    for (long long w = 0; w < walks; ++w) {
      W cur = (w & 1) ? elected : s0;
      for (long long len = 1;; ++len) {
        if (done.insert(packed(cur)).second) c.state(cur);
        if (len >= walk_depth) break;
        std::vector<W> in;
        for (int k = 0; k < S::NI; ++k) {
          W t; u32 err = 0;
          if (S::apply(cur, k, t, err) < 0) continue;
          S::all_logs_next(cur, t.allLogs);
          if (S::in_model(t, m.rt) && !S::violated(t, m.rt.invariants)) in.push_back(t);
        }
        if (in.empty()) break;
        const u64 key = sim_step_key(seed, (u64)w, (u32)(len - 1));
        size_t keep = 0;
        for (size_t j = 1; j <= in.size(); ++j) if (sim_take(key, (u32)j)) keep = j - 1;
        cur = in[keep];
      }
    }
    c.print();
    return 0;
  }

  if (check) {   // the unsymmetric BFS: the reachable set is closed under Permutations(Server)
    Check c; c.seed = seed;
    std::set<Words> seen;
    std::vector<W> frontier{s0};
    seen.insert(packed(s0));
    while (!frontier.empty()) {
      std::vector<W> next;
      for (const W& s : frontier) {
        c.state(s);
        for (int k = 0; k < S::NI; ++k) {
          W t; u32 err = 0;
          if (S::apply(s, k, t, err) < 0) continue;
          S::all_logs_next(s, t.allLogs);
          if (S::in_model(t, m.rt) && seen.insert(packed(t)).second) next.push_back(t);
        }
      }
      frontier.swap(next);
    }
    c.print();
    return 0;
  }

  // the symmetric single-worker FIFO BFS
  auto first_bad = [&](const W& t) -> std::string {
    for (auto& n : m.inv_names) if (S::violated(t, orig_inv_bit(n.c_str()))) return n;
    return "";
  };
  std::unordered_set<u64> seen;
  struct Node { W s; long long parent; };
  std::vector<Node> store;
  long long generated = 1, gen_act[OA_NACT] = {0}, dist_act[OA_NACT] = {0};
  std::vector<long long> levels;
  std::string verdict = "OK", violated;
  size_t trace_len = 0;
  int depth = 0;
  u32 err = 0;
  std::vector<long long> frontier;
  if (S::in_model(s0, m.rt)) {
    seen.insert(S::fp_sym(s0, seed));
    store.push_back({s0, -1}); frontier.push_back(0);
    depth = 1; levels.push_back(1);
  }
  auto chain = [&](long long idx) { size_t n = 0; while (idx >= 0) { ++n; idx = store[idx].parent; } return n; };
  int level = 1;
  bool stop = false;
  while (!frontier.empty() && !stop) {
    if (max_depth && level >= max_depth) { verdict = "DEPTH_LIMIT"; break; }
    std::vector<long long> next;
    for (size_t fi = 0; fi < frontier.size() && !stop; ++fi) {
      const long long idx = frontier[fi];
      const W s = store[idx].s;
      std::vector<std::pair<int, W>> succ;
      for (int k = 0; k < S::NI; ++k) {
        W t;
        const int act = S::apply(s, k, t, err);
        if (act < 0) continue;
        S::all_logs_next(s, t.allLogs);
        succ.push_back({act, t});
      }
      generated += (long long)succ.size();
      for (auto& su : succ) {
        const int act = su.first; const W& t = su.second;
        gen_act[act]++;
        const bool im = S::in_model(t, m.rt);
        const bool isnew = im && seen.insert(S::fp_sym(t, seed)).second;
        if (isnew) { store.push_back({t, idx}); next.push_back((long long)store.size() - 1); dist_act[act]++; }
        if (isnew || !im) {
          const std::string bad = first_bad(t);
          if (!bad.empty()) {
            verdict = "INVARIANT_VIOLATION"; violated = bad;
            trace_len = chain(idx) + 1; depth = level + 1;
            stop = true; break;
          }
        }
      }
    }
    if (stop) break;
    if (!next.empty()) { level++; depth = level; levels.push_back((long long)next.size()); }
    frontier.swap(next);
  }
  std::printf("{\"verdict\": \"%s\", \"violated\": \"%s\", \"generated\": %lld, \"distinct\": %zu, \"depth\": %d, \"err\": %u, \"levels\": [",
              verdict.c_str(), violated.c_str(), generated, seen.size(), depth, err);
  for (size_t q = 0; q < levels.size(); ++q) std::printf("%s%lld", q ? ", " : "", levels[q]);
  std::printf("], \"actions\": {");
  for (int k = 0; k < OA_NACT; ++k) std::printf("%s\"%s\": [%lld, %lld]", k ? ", " : "", kOrigActNames[k], gen_act[k], dist_act[k]);
  std::printf("}, \"trace_len\": %zu}\n", trace_len);
  return 0;
}
