// TEST HARNESS ONLY (never part of the product).  The log- and commit-safety invariants of
// configs/raft_original_safety_mc.tla on the host, over the header the gfx950 kernels compile
// (raft-tla_amd/csrc/orig_spec.h): the packed evaluation WithSafety<S>::violated (masked log-word
// compares, popcounts) against a literal evaluator of each definition over an unpacked state (plain
// loops, every subset of Server enumerated for Quorum, SubSeq compared element by element).
//
//   orig_safety_host CFG [--mutations M] [--seed S]
//       the unsymmetric BFS of the cfg (its constraints; its invariants are not consulted).  Compared
//       bit for bit: every reachable state, every generated successor (out-of-model ones included:
//       the kernels check those too) and M mutated copies of every reachable state (seeded; one to
//       three of commitIndex[i], a log entry, the length of a log, votedFor[i], state[i],
//       currentTerm[i] redrawn within their canonical ranges).
//       Frame check: on every reachable (state, successor, action), an invariant that holds in the
//       parent and fails in the successor must be in WithSafety<S>::inv_frame(action).
//       One JSON line: states, compared, disagreements, frame_checked, frame_bad, and per invariant
//       [times true, times false] over the compared states.
// Shape: -DSHAPE_N=.. -DSHAPE_NV=.. -DSHAPE_MT=.. -DSHAPE_ML=.. -DSHAPE_MK=..
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../../raft-tla_amd/csrc/orig_text.h"

using namespace rmc;
using S = Orig<SHAPE_N, SHAPE_NV, SHAPE_MT, SHAPE_ML, SHAPE_MK>;
using SS = WithSafety<S>;
using W = S::Work;
using Words = std::vector<u32>;
constexpr int N = S::N;
constexpr int NIL = S::N;

static Words packed(const W& s) { u32 a[S::NW]; S::pack(s, a); return Words(a, a + S::NW); }

// ---------------------------------------------------------------- the literal evaluator
struct Entry { int term, value; bool operator==(const Entry& o) const { return term == o.term && value == o.value; } };
using Log = std::vector<Entry>;   // log[n] is Log[n - 1]
struct Plain {
  int currentTerm[N], state[N], votedFor[N], commitIndex[N];   // state: S::F / S::C / S::L; votedFor: server or NIL
  Log log[N];
};
static Plain unpacked(const W& t) {
  Plain p;
  for (int i = 0; i < N; ++i) {
    p.currentTerm[i] = S::g_term(t, i); p.state[i] = S::g_st(t, i); p.votedFor[i] = S::g_voted(t, i); p.commitIndex[i] = S::g_commit(t, i);
    const u32 lw = t.log.v[i];
    for (int n = 0; n < S::llen(lw); ++n) p.log[i].push_back({S::eterm(S::lent(lw, n)), S::evalue(S::lent(lw, n))});
  }
  return p;
}
static int Len(const Log& s) { return (int)s.size(); }
static Log SubSeq(const Log& s, int a, int b) { Log r; for (int n = a; n <= b; ++n) r.push_back(s[n - 1]); return r; }
static bool SeqEq(const Log& s, const Log& t) {
  if (s.size() != t.size()) return false;
  for (size_t n = 0; n < s.size(); ++n) if (!(s[n] == t[n])) return false;
  return true;
}
static int LastTerm(const Log& s) { return s.empty() ? 0 : s.back().term; }
static int CommittedLen(const Plain& p, int i) { return p.commitIndex[i] <= Len(p.log[i]) ? p.commitIndex[i] : Len(p.log[i]); }
static Log Committed(const Plain& p, int i) { return SubSeq(p.log[i], 1, CommittedLen(p, i)); }
static bool PrefixOf(const Log& s, const Log& t) { return Len(s) <= Len(t) && SeqEq(SubSeq(t, 1, Len(s)), s); }
static int MaxOrZero(const std::set<int>& s) { return s.empty() ? 0 : *s.rbegin(); }
// Quorum == {i \in SUBSET(Server) : Cardinality(i) * 2 > Cardinality(Server)}, every subset enumerated
static std::vector<u32> Quorum() {
  std::vector<u32> q;
  for (u32 sub = 0; sub < (1u << N); ++sub) if (__builtin_popcount(sub) * 2 > N) q.push_back(sub);
  return q;
}
static bool InQuorum(u32 set) { for (u32 q : Quorum()) if (q == set) return true; return false; }

static u32 literal(const Plain& p) {
  u32 bad = 0;
  {   // CommitWithinLog
    bool ok = true;
    for (int i = 0; i < N; ++i) ok = ok && p.commitIndex[i] <= Len(p.log[i]);
    if (!ok) bad |= OI_CommitWithinLog;
  }
  {   // LeaderVotesQuorum
    bool ok = true;
    for (int i = 0; i < N; ++i) {
      if (p.state[i] != (int)S::L) continue;
      u32 set = 0;
      for (int j = 0; j < N; ++j)
        if (p.currentTerm[j] > p.currentTerm[i] || (p.currentTerm[j] == p.currentTerm[i] && p.votedFor[j] == i)) set |= 1u << j;
      ok = ok && InQuorum(set);
    }
    if (!ok) bad |= OI_LeaderVotesQuorum;
  }
  {   // CandidateTermNotInLog
    bool ok = true;
    for (int i = 0; i < N; ++i) {
      u32 set = 0;
      for (int j = 0; j < N; ++j)
        if (p.currentTerm[j] == p.currentTerm[i] && (p.votedFor[j] == i || p.votedFor[j] == NIL)) set |= 1u << j;
      if (!(p.state[i] == (int)S::C && InQuorum(set))) continue;
      for (int j = 0; j < N; ++j)
        for (int n = 1; n <= Len(p.log[j]); ++n) ok = ok && p.log[j][n - 1].term != p.currentTerm[i];
    }
    if (!ok) bad |= OI_CandidateTermNotInLog;
  }
  {   // LeaderHasLatestOfTerm
    bool ok = true;
    for (int i = 0; i < N; ++i) {
      if (p.state[i] != (int)S::L) continue;
      for (int j = 0; j < N; ++j) {
        std::set<int> a, b;
        for (int n = 1; n <= Len(p.log[i]); ++n) if (p.log[i][n - 1].term == p.currentTerm[i]) a.insert(n);
        for (int n = 1; n <= Len(p.log[j]); ++n) if (p.log[j][n - 1].term == p.currentTerm[i]) b.insert(n);
        ok = ok && MaxOrZero(a) >= MaxOrZero(b);
      }
    }
    if (!ok) bad |= OI_LeaderHasLatestOfTerm;
  }
  {   // VotesGrantedInv
    bool ok = true;
    for (int i = 0; i < N; ++i)
      for (int j = 0; j < N; ++j)
        if (p.votedFor[i] == j) ok = ok && PrefixOf(Committed(p, i), p.log[j]);
    if (!ok) bad |= OI_VotesGrantedInv;
  }
  {   // QuorumLogInv
    bool ok = true;
    for (int i = 0; i < N; ++i)
      for (u32 q : Quorum()) {
        bool some = false;
        for (int j = 0; j < N; ++j) if ((q >> j) & 1u) some = some || PrefixOf(Committed(p, i), p.log[j]);
        ok = ok && some;
      }
    if (!ok) bad |= OI_QuorumLogInv;
  }
  {   // MoreUpToDateCorrect
    bool ok = true;
    for (int i = 0; i < N; ++i)
      for (int j = 0; j < N; ++j) {
        const bool upto = LastTerm(p.log[i]) > LastTerm(p.log[j]) ||
                          (LastTerm(p.log[i]) == LastTerm(p.log[j]) && Len(p.log[i]) >= Len(p.log[j]));
        if (upto) ok = ok && PrefixOf(Committed(p, j), p.log[i]);
      }
    if (!ok) bad |= OI_MoreUpToDateCorrect;
  }
  {   // LeaderCompleteness
    bool ok = true;
    for (int i = 0; i < N; ++i)
      for (int idx = 1; idx <= CommittedLen(p, i); ++idx)
        for (int l = 0; l < N; ++l)
          if (p.state[l] == (int)S::L && p.currentTerm[l] > p.log[i][idx - 1].term)
            ok = ok && idx <= Len(p.log[l]) && p.log[l][idx - 1] == p.log[i][idx - 1];
    if (!ok) bad |= OI_LeaderCompleteness;
  }
  {   // StateMachineSafety
    bool ok = true;
    for (int i = 0; i < N; ++i)
      for (int j = 0; j < N; ++j)
        for (int n = 1; n <= CommittedLen(p, i) && n <= CommittedLen(p, j); ++n) ok = ok && p.log[i][n - 1] == p.log[j][n - 1];
    if (!ok) bad |= OI_StateMachineSafety;
  }
  {   // AllHaveCommitted_false
    bool ok = true;
    for (int i = 0; i < N; ++i)
      for (int j = 0; j < N; ++j) ok = ok && PrefixOf(Committed(p, i), p.log[j]);
    if (!ok) bad |= OI_AllHaveCommitted_false;
  }
  return bad;
}

// ---------------------------------------------------------------- mutation (splitmix64 draws)
static u64 rng_state = 1;
static u64 draw() {
  u64 z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static int below(int n) { return (int)(draw() % (u64)n); }
static void mutate(W& t) {
  const int changes = 1 + below(3);
  for (int c = 0; c < changes; ++c) {
    const int i = below(N);
    switch (below(6)) {
      case 0: fset<S::CIB>(t.commit, i, (u32)below(S::ML + 1)); break;                 // commitIndex[i] in 0..MaxLogLen
      case 1: {                                                                        // one entry of log[i] redrawn
        const u32 lw = t.log.v[i];
        const int n = S::llen(lw);
        if (n == 0) break;
        const int p = below(n);
        const u32 m = (u32)lomask(S::EB) << (S::LLB + p * S::EB);
        t.log.v[i] = (lw & ~m) | ((u32)(1 + below(S::E)) << (S::LLB + p * S::EB));
        break;
      }
      case 2: {                                                                        // Len(log[i]) redrawn in 0..MaxLogLen
        const int n = below(S::ML + 1);
        u32 lw = 0;
        for (int p = 0; p < n; ++p) {
          const int old = p < S::llen(t.log.v[i]) ? S::lent(t.log.v[i], p) : 0;
          lw = S::lappend(lw, old ? old : 1 + below(S::E));
        }
        t.log.v[i] = lw;
        break;
      }
      case 3: fset<S::VB>(t.voted, i, (u32)below(N + 1)); break;                       // votedFor[i] in Server \cup {Nil}
      case 4: fset<2>(t.st, i, (u32)below(3)); break;                                  // state[i]
      default: fset<S::TB>(t.term, i, (u32)(1 + below(S::MT))); break;                 // currentTerm[i] in 1..MaxTerm
    }
  }
}

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: orig_safety_host CFG [--mutations M] [--seed S]\n"); return 2; }
  CfgFile cfg = parse_cfg_text(read_text_file(argv[1]));
  cfg.invariant_defs.assign(cfg.invariants.size(), "defined");   // the harness takes the names on trust
  const OrigModel m = resolve_orig_model(cfg);
  long long mutations = 0;
  for (int a = 2; a < argc; ++a) {
    const std::string k = argv[a];
    if (k == "--mutations" && a + 1 < argc) mutations = std::atoll(argv[++a]);
    else if (k == "--seed" && a + 1 < argc) rng_state = std::strtoull(argv[++a], nullptr, 0);
    else { std::fprintf(stderr, "unknown argument %s\n", argv[a]); return 2; }
  }
  const u32 ALL = OI_ElectionSafety | OI_LogMatching | OI_SAFETY_MASK;
  long long states = 0, compared = 0, disagreements = 0, frame_checked = 0, frame_bad = 0;
  long long holds[kOrigInvCount] = {0}, fails[kOrigInvCount] = {0};
  auto compare = [&](const W& t) {
    const u32 got = SS::violated(t, OI_SAFETY_MASK), want = literal(unpacked(t));
    ++compared;
    if (got != want) {
      if (++disagreements <= 5) std::fprintf(stderr, "disagreement: packed %#x literal %#x\n%s\n", got, want, orig_state_text<S>(m, t, true).c_str());
    }
    for (int k = 0; k < kOrigInvCount; ++k)
      if (OI_SAFETY_MASK & (1u << k)) ((want >> k) & 1u ? fails[k] : holds[k])++;
  };
  W s0; S::init(s0);
  std::set<Words> seen;
  std::vector<W> frontier{s0};
  seen.insert(packed(s0));
  while (!frontier.empty()) {
    std::vector<W> next;
    for (const W& s : frontier) {
      ++states;
      compare(s);
      for (long long q = 0; q < mutations; ++q) { W t = s; mutate(t); compare(t); }
      const u32 parent_bad = SS::violated(s, ALL);
      for (int k = 0; k < S::NI; ++k) {
        W t; u32 err = 0;
        const int act = S::apply(s, k, t, err);
        if (act < 0) continue;
        S::all_logs_next(s, t.allLogs);
        const bool im = S::in_model(t, m.rt);
        if (!im) compare(t);   // (the in-model ones are compared as reachable states)
        ++frame_checked;
        if (SS::violated(t, ALL) & ~parent_bad & ~SS::inv_frame(act)) {
          if (++frame_bad <= 5) std::fprintf(stderr, "frame: %s\n%s\n", kOrigActNames[act], orig_state_text<S>(m, t, true).c_str());
        }
        if (im && seen.insert(packed(t)).second) next.push_back(t);
      }
    }
    frontier.swap(next);
  }
  std::printf("{\"states\": %lld, \"compared\": %lld, \"disagreements\": %lld, \"frame_checked\": %lld, \"frame_bad\": %lld, \"invariants\": {",
              states, compared, disagreements, frame_checked, frame_bad);
  bool first = true;
  for (int k = 0; k < kOrigInvCount; ++k)
    if (OI_SAFETY_MASK & (1u << k)) { std::printf("%s\"%s\": [%lld, %lld]", first ? "" : ", ", kOrigInvNames[k], holds[k], fails[k]); first = false; }
  std::printf("}}\n");
  return 0;
}
