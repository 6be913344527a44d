// TEST HARNESS ONLY (never part of the product).  The action properties ([][A]_vars) of
// configs/raft_original_actions_mc.tla on the host, over the header the gfx950 kernels compile
// (raft-tla_amd/csrc/orig_spec.h): the packed evaluation S::violated_action (field compares, masked
// log-word compares, Restart(i) as word compares) and S::act_frame against a literal evaluator of each
// definition over an unpacked pair of states (sequences element by element, Restart(i) conjunct by
// conjunct over all variables), plus single-threaded mirrors of the BFS and of simulation mode that
// check the properties with the literal evaluator.
//
//   orig_actions_host check CFG [--mutations M] [--seed S]
//       the unsymmetric BFS of the cfg (its constraints; its invariants and properties are not consulted).
//       On every reachable transition (s, t, k) -- out-of-model successors included -- and on M mutated
//       copies of t per transition (seeded; one to three of currentTerm[i], votedFor[i], state[i],
//       commitIndex[i], a log entry, the length of a log redrawn), the packed mask of all six equals the
//       literal one.  Frame check, on every reachable transition: the packed mask under act_frame(action)
//       equals the full one.  One JSON line: states, transitions, compared, disagreements, frame_checked,
//       frame_bad, restart_steps, and per property [times held, times violated] over the compared pairs.
//   orig_actions_host bfs CFG [--no-inv-oom]
//       single-worker FIFO BFS with tests/native/orig_host_bfs.cpp's contract plus DESIGN.md §14's rules for
//       the cfg's PROPERTIES (literal evaluator); the oracle's JSON fields.
//   orig_actions_host sim CFG SEED NUM DEPTH BATCH [--walk W] [--no-inv-oom]
//       tests/native/orig_sim_host.cpp's walker with the property check on every generated successor.
// Shape: -DSHAPE_N=.. -DSHAPE_NV=.. -DSHAPE_MT=.. -DSHAPE_ML=.. -DSHAPE_MK=..
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../raft-tla_amd/csrc/orig_text.h"
#include "../../raft-tla_amd/csrc/sim_rng.h"

using namespace rmc;
using S = Orig<SHAPE_N, SHAPE_NV, SHAPE_MT, SHAPE_ML, SHAPE_MK>;
using W = S::Work;
constexpr int N = S::N;
constexpr int NIL = S::N;
constexpr u32 ALL_PROPS = (1u << kOrigPropCount) - 1u;

// ---------------------------------------------------------------- the literal evaluator
struct Entry { int term, value; bool operator==(const Entry& o) const { return term == o.term && value == o.value; } };
struct Log { int n = 0; Entry e[S::ML + 2]; };   // log[k] is e[k - 1]
struct Plain {
  int currentTerm[N], state[N], votedFor[N], commitIndex[N];   // state: S::F / S::C / S::L; votedFor: server or NIL
  Log log[N];
  u32 votesResponded[N], votesGranted[N];   // server sets
  u64 voterLog[N];                          // row i: per voter a presence bit and the index of its log
  int nextIndex[N][N], matchIndex[N][N];
  std::vector<u64> messages, elections;     // the bag's (message, count) entries / the election records, sorted
};
static Plain unpacked(const W& t) {
  Plain p;
  for (int i = 0; i < N; ++i) {
    p.currentTerm[i] = S::g_term(t, i); p.state[i] = S::g_st(t, i); p.votedFor[i] = S::g_voted(t, i); p.commitIndex[i] = S::g_commit(t, i);
    const u32 lw = t.log.v[i];
    p.log[i].n = S::llen(lw);
    for (int k = 0; k < p.log[i].n; ++k) p.log[i].e[k] = {S::eterm(S::lent(lw, k)), S::evalue(S::lent(lw, k))};
    p.votesResponded[i] = S::row_bits(t.vresp, i); p.votesGranted[i] = S::row_bits(t.vgrant, i);
    p.voterLog[i] = (u64)t.vl.v[i];
    for (int j = 0; j < N; ++j) { p.nextIndex[i][j] = S::g_ni(t, i, j); p.matchIndex[i][j] = S::g_mi(t, i, j); }
  }
  for (int k = 0; k < S::MK + 1; ++k) if (t.bag.v[k] != S::BEMPTY) p.messages.push_back((u64)t.bag.v[k]);
  for (int k = 0; k < S::EMAX; ++k) if (t.el[k] != S::EMPTY) p.elections.push_back(t.el[k]);
  return p;
}
static int Len(const Log& s) { return s.n; }
static Log SubSeq(const Log& s, int a, int b) { Log r; for (int k = a; k <= b; ++k) r.e[r.n++] = s.e[k - 1]; return r; }
static bool SeqEq(const Log& s, const Log& t) {
  if (s.n != t.n) return false;
  for (int k = 0; k < s.n; ++k) if (!(s.e[k] == t.e[k])) return false;
  return true;
}
static int CommittedLen(const Plain& p, int i) { return p.commitIndex[i] <= Len(p.log[i]) ? p.commitIndex[i] : Len(p.log[i]); }
static Log Committed(const Plain& p, int i) { return SubSeq(p.log[i], 1, CommittedLen(p, i)); }
static bool PrefixOf(const Log& s, const Log& t) { return Len(s) <= Len(t) && SeqEq(SubSeq(t, 1, Len(s)), s); }

// Restart(i) (raft_original.tla:166-174) as a formula over (p, q), one conjunct per line of the definition
static bool Restart(const Plain& p, const Plain& q, int i) {
  bool ok = true;
  for (int j = 0; j < N; ++j) ok = ok && q.state[j] == (j == i ? (int)S::F : p.state[j]);                  // state' = [state EXCEPT ![i] = Follower]
  for (int j = 0; j < N; ++j) ok = ok && q.votesResponded[j] == (j == i ? 0u : p.votesResponded[j]);       // votesResponded'
  for (int j = 0; j < N; ++j) ok = ok && q.votesGranted[j] == (j == i ? 0u : p.votesGranted[j]);           // votesGranted'
  for (int j = 0; j < N; ++j) ok = ok && q.voterLog[j] == (j == i ? 0ull : p.voterLog[j]);                 // voterLog'
  for (int j = 0; j < N; ++j)
    for (int k = 0; k < N; ++k) ok = ok && q.nextIndex[j][k] == (j == i ? 1 : p.nextIndex[j][k]);          // nextIndex'
  for (int j = 0; j < N; ++j)
    for (int k = 0; k < N; ++k) ok = ok && q.matchIndex[j][k] == (j == i ? 0 : p.matchIndex[j][k]);        // matchIndex'
  for (int j = 0; j < N; ++j) ok = ok && q.commitIndex[j] == (j == i ? 0 : p.commitIndex[j]);              // commitIndex'
  ok = ok && q.messages == p.messages;                                                                    // UNCHANGED <<messages,
  for (int j = 0; j < N; ++j) ok = ok && q.currentTerm[j] == p.currentTerm[j];                             //   currentTerm,
  for (int j = 0; j < N; ++j) ok = ok && q.votedFor[j] == p.votedFor[j];                                   //   votedFor,
  for (int j = 0; j < N; ++j) ok = ok && SeqEq(q.log[j], p.log[j]);                                        //   log,
  ok = ok && q.elections == p.elections;                                                                  //   elections>>
  return ok;
}

// the OP_* bits of the properties the step (p, q) violates ([A]_vars: a stuttering step satisfies each A)
static u32 literal(const Plain& p, const Plain& q) {
  u32 bad = 0;
  for (int i = 0; i < N; ++i) {
    if (!(q.currentTerm[i] >= p.currentTerm[i])) bad |= OP_TermsMonotonic;
    if (q.currentTerm[i] == p.currentTerm[i] && p.votedFor[i] != NIL && !(q.votedFor[i] == p.votedFor[i])) bad |= OP_OneVotePerTerm;
    if (p.state[i] == (int)S::L && q.state[i] == (int)S::L && !PrefixOf(p.log[i], q.log[i])) bad |= OP_LeaderAppendOnly;
    if (!PrefixOf(Committed(p, i), q.log[i])) bad |= OP_CommittedNeverLost;
    if (!(q.commitIndex[i] >= p.commitIndex[i] || Restart(p, q, i))) bad |= OP_CommitIndexMonotonic;
    if (p.state[i] == (int)S::L && !(q.state[i] == (int)S::L)) bad |= OP_LeaderNeverStepsDown_false;
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

struct Key { u32 w[S::NW]; bool operator==(const Key& o) const { return std::memcmp(w, o.w, sizeof w) == 0; } };
struct KH { size_t operator()(const Key& k) const { return (size_t)fp64(k.w, 1); } };
static Key key_of(const W& s) { Key k; S::pack(s, k.w); return k; }

static std::string jstr(const std::string& s) {
  std::string o = "\"";
  for (char c : s) { if (c == '"' || c == '\\') o += '\\'; o += c; }
  return o + "\"";
}

static OrigModel model_of(const char* path) {
  CfgFile cfg = parse_cfg_text(read_text_file(path));
  cfg.invariant_defs.assign(cfg.invariants.size(), "defined");   // the harness takes the names on trust
  cfg.property_defs.assign(cfg.properties.size(), "defined");
  return resolve_orig_model(cfg);
}

// first listed property (cfg order) the step violates, by the literal evaluator; "" if none
static std::string first_prop(const OrigModel& m, const W& s, const W& t) {
  if (m.prop_names.empty()) return "";
  const u32 bad = literal(unpacked(s), unpacked(t));
  for (auto& n : m.prop_names) if (bad & orig_prop_bit(n.c_str())) return n;
  return "";
}
static std::string first_inv(const OrigModel& m, const W& t) {
  using SS = WithSafety<S>;
  for (auto& n : m.inv_names) if (SS::violated(t, orig_inv_bit(n.c_str()))) return n;
  return "";
}

// ---------------------------------------------------------------- check
static int main_check(const OrigModel& m, long long mutations) {
  long long states = 0, transitions = 0, compared = 0, disagreements = 0, frame_checked = 0, frame_bad = 0, restart_steps = 0;
  long long holds[kOrigPropCount] = {0}, fails[kOrigPropCount] = {0};
  auto compare = [&](const Plain& ps, const W& s, const W& t, int k) {
    const u32 got = S::violated_action(s, t, k, ALL_PROPS), want = literal(ps, unpacked(t));
    ++compared;
    if (got != want && ++disagreements <= 5)
      std::fprintf(stderr, "disagreement at instance %d: packed %#x literal %#x\n%s\n%s\n", k, got, want,
                   orig_state_text<S>(m, s, true).c_str(), orig_state_text<S>(m, t, true).c_str());
    for (int q = 0; q < kOrigPropCount; ++q) ((want >> q) & 1u ? fails[q] : holds[q])++;
  };
  W s0; S::init(s0);
  std::unordered_map<Key, int, KH> seen;
  std::vector<W> frontier{s0};
  seen.emplace(key_of(s0), 0);
  while (!frontier.empty()) {
    std::vector<W> next;
    for (const W& s : frontier) {
      ++states;
      const Plain ps = unpacked(s);
      for (int k = 0; k < S::NI; ++k) {
        W t; u32 err = 0;
        const int act = S::apply(s, k, t, err);
        if (act < 0) continue;
        S::all_logs_next(s, t.allLogs);
        ++transitions;
        compare(ps, s, t, k);
        for (long long q = 0; q < mutations; ++q) { W u = t; mutate(u); compare(ps, s, u, k); }
        ++frame_checked;
        const u32 full = S::violated_action(s, t, k, ALL_PROPS), framed = S::violated_action(s, t, k, ALL_PROPS & S::act_frame(act));
        if (full != framed && ++frame_bad <= 5)
          std::fprintf(stderr, "frame: %s full %#x framed %#x\n%s\n%s\n", kOrigActNames[act], full, framed,
                       orig_state_text<S>(m, s, true).c_str(), orig_state_text<S>(m, t, true).c_str());
        if (act == OA_Restart) {   // the formula, not the action's name: Restart(i) holds of every step of instance i
          ++restart_steps;
          if (!Restart(ps, unpacked(t), k)) ++frame_bad;
        }
        if (S::in_model(t, m.rt) && seen.emplace(key_of(t), 0).second) next.push_back(t);
      }
    }
    frontier.swap(next);
  }
  std::printf("{\"states\": %lld, \"transitions\": %lld, \"compared\": %lld, \"disagreements\": %lld, \"frame_checked\": %lld, "
              "\"frame_bad\": %lld, \"restart_steps\": %lld, \"properties\": {",
              states, transitions, compared, disagreements, frame_checked, frame_bad, restart_steps);
  for (int q = 0; q < kOrigPropCount; ++q) std::printf("%s\"%s\": [%lld, %lld]", q ? ", " : "", kOrigPropNames[q], holds[q], fails[q]);
  std::printf("}}\n");
  return 0;
}

// ---------------------------------------------------------------- bfs
static int main_bfs(const OrigModel& m, bool inv_oom) {
  std::unordered_map<Key, long long, KH> seen;
  std::vector<W> store;
  struct Node { long long parent; int act; };
  std::vector<Node> nodes;
  long long generated = 1, gen_act[OA_NACT] = {0}, dist_act[OA_NACT] = {0}, left = 0;
  std::vector<long long> levels;
  std::string verdict = "OK", violated;
  std::vector<std::pair<int, W>> trace;
  auto build_trace = [&](long long idx, int last_act, const W* last) {
    std::vector<std::pair<int, W>> tr;
    if (last) tr.push_back({last_act, *last});
    while (idx >= 0) { tr.push_back({nodes[idx].act, store[idx]}); idx = nodes[idx].parent; }
    std::reverse(tr.begin(), tr.end());
    trace = tr;
  };
  W s0; S::init(s0);
  int depth = 0, level = 1;
  std::vector<long long> frontier;
  if (S::in_model(s0, m.rt)) {
    seen.emplace(key_of(s0), 0); store.push_back(s0); nodes.push_back({-1, -1}); frontier.push_back(0);
    depth = 1; levels.push_back(1);
    const std::string bad = first_inv(m, s0);   // Init has no incoming step: no property can fail on it
    if (!bad.empty()) { verdict = "INVARIANT_VIOLATION"; violated = bad; build_trace(0, -1, nullptr); frontier.clear(); }
  }
  while (!frontier.empty()) {
    std::vector<long long> next;
    bool stop = false;
    for (size_t fi = 0; fi < frontier.size() && !stop; ++fi) {
      const long long idx = frontier[fi];
      const W s = store[idx];
      std::vector<std::pair<int, W>> succ;
      u32 e1 = 0;
      for (int k = 0; k < S::NI; ++k) {
        W t; const int act = S::apply(s, k, t, e1);
        if (act < 0) continue;
        S::all_logs_next(s, t.allLogs);
        succ.push_back({act, t});
      }
      if (e1) { std::printf("{\"error\": \"successor-function error flag %u\"}\n", e1); return 1; }
      generated += (long long)succ.size();
      for (auto& su : succ) {
        const int act = su.first; const W& t = su.second;
        gen_act[act]++;
        const bool im = S::in_model(t, m.rt);
        bool isnew = false;
        if (im && seen.emplace(key_of(t), (long long)store.size()).second) {
          isnew = true;
          store.push_back(t); nodes.push_back({idx, act}); next.push_back((long long)store.size() - 1);
          dist_act[act]++;
        }
        std::string bad, kind;
        if (isnew || (!im && inv_oom)) { bad = first_inv(m, t); kind = "INVARIANT_VIOLATION"; }   // invariants before implied actions
        if (bad.empty() && (im || inv_oom)) { bad = first_prop(m, s, t); kind = "ACTION_PROPERTY_VIOLATION"; }
        if (!bad.empty()) {
          verdict = kind; violated = bad;
          if (isnew) build_trace((long long)store.size() - 1, -1, nullptr); else build_trace(idx, act, &t);
          depth = level + 1;
          left = (long long)(frontier.size() - fi - 1 + next.size());
          stop = true; break;
        }
      }
    }
    if (stop) break;
    if (!next.empty()) { level++; depth = level; levels.push_back((long long)next.size()); }
    frontier.swap(next);
  }
  std::printf("{\"verdict\": %s, \"violated\": %s, \"generated\": %lld, \"distinct\": %zu, \"left_on_queue\": %lld, \"depth\": %d, \"levels\": [",
              jstr(verdict).c_str(), jstr(violated).c_str(), generated, seen.size(), left, depth);
  for (size_t q = 0; q < levels.size(); ++q) std::printf("%s%lld", q ? ", " : "", levels[q]);
  std::printf("], \"actions\": {");
  for (int k = 0; k < OA_NACT; ++k) std::printf("%s\"%s\": [%lld, %lld]", k ? ", " : "", kOrigActNames[k], gen_act[k], dist_act[k]);
  std::printf("}, \"trace_len\": %zu, \"trace\": [", trace.size());
  for (size_t q = 0; q < trace.size(); ++q)
    std::printf("%s{\"action\": %s, \"state\": %s}", q ? ", " : "", jstr(trace[q].first < 0 ? "Init" : kOrigActNames[trace[q].first]).c_str(),
                jstr(orig_state_text<S>(m, trace[q].second, false)).c_str());
  std::printf("]}\n");
  return 0;
}

// ---------------------------------------------------------------- sim (orig_sim_host.cpp's rules + the properties)
struct Cand { int k, act; W t; };
struct Walk {
  std::vector<W> states;
  long long steps = 0;
  long long gen[OA_NACT] = {0};
  bool event = false;
  int ev_inst = -1;
};
static Walk run_walk(const OrigModel& m, bool inv_oom, u64 seed, u64 walk, int depth) {
  Walk out;
  W cur;
  S::init(cur);
  out.states.push_back(cur);
  while ((int)out.states.size() < depth) {
    const u32 step = (u32)out.states.size() - 1;
    ++out.steps;
    std::vector<Cand> inmodel;
    int viol = -1;
    W viol_state = cur;
    for (int k = 0; k < S::NI; ++k) {
      Cand c; c.k = k;
      u32 err = 0;
      c.act = S::apply(cur, k, c.t, err);
      if (c.act < 0) continue;
      if (err) { std::fprintf(stderr, "successor-function error flag %u (walk %llu)\n", err, (unsigned long long)walk); std::exit(4); }
      S::all_logs_next(cur, c.t.allLogs);
      ++out.gen[c.act];
      const bool in = S::in_model(c.t, m.rt);
      if ((in || inv_oom) && viol < 0 && (!first_inv(m, c.t).empty() || !first_prop(m, cur, c.t).empty())) { viol = k; viol_state = c.t; }
      if (in) inmodel.push_back(c);
    }
    if (viol >= 0) {
      out.states.push_back(viol_state);
      out.event = true; out.ev_inst = viol;
      break;
    }
    if (inmodel.empty()) break;
    const u64 key = sim_step_key(seed, walk, step);
    size_t keep = 0;
    for (size_t j = 1; j <= inmodel.size(); ++j)
      if (sim_take(key, (u32)j)) keep = j - 1;
    cur = inmodel[keep].t;
    out.states.push_back(cur);
  }
  return out;
}
static int main_sim(const OrigModel& m, int argc, char** argv) {
  if (argc < 7) return 2;
  const u64 seed = std::strtoull(argv[3], nullptr, 0);
  const long long num = std::atoll(argv[4]);
  const int depth = std::atoi(argv[5]);
  const long long batch = std::atoll(argv[6]);
  long long one = -1;
  bool inv_oom = true;
  for (int a = 7; a < argc; ++a) {
    if (!std::strcmp(argv[a], "--walk") && a + 1 < argc) one = std::atoll(argv[++a]);
    else if (!std::strcmp(argv[a], "--no-inv-oom")) inv_oom = false;
    else return 2;
  }
  if (one >= 0) {
    const Walk w = run_walk(m, inv_oom, seed, (u64)one, depth);
    for (const W& st : w.states) std::printf("%s\n", orig_state_text<S>(m, st, false).c_str());
    return 0;
  }
  long long generated = 0, steps = 0, walks = 0, longest = 1, gen[OA_NACT] = {0};
  bool have = false;
  long long ev_len = 0, ev_walk = 0, ev_inst = 0;
  for (long long w0 = 0; w0 < num && !have; w0 += batch) {
    const long long n = std::min(batch, num - w0);
    for (long long w = w0; w < w0 + n; ++w) {
      const Walk r = run_walk(m, inv_oom, seed, (u64)w, depth);
      steps += r.steps;
      for (int a = 0; a < OA_NACT; ++a) { gen[a] += r.gen[a]; generated += r.gen[a]; }
      longest = std::max<long long>(longest, (long long)r.states.size());
      if (r.event) {
        const long long len = (long long)r.states.size();
        if (!have || len < ev_len) { ev_len = len; ev_walk = w; ev_inst = r.ev_inst; }   // minimum (length, walk, instance)
        have = true;
      }
    }
    walks += n;
  }
  std::printf("{\"generated\": %lld, \"steps\": %lld, \"walks\": %lld, \"depth\": %lld, \"actions\": {", generated, steps, walks, longest);
  for (int a = 0; a < OA_NACT; ++a) std::printf("%s\"%s\": %lld", a ? ", " : "", kOrigActNames[a], gen[a]);
  std::printf("}, \"event\": ");
  if (have) std::printf("{\"length\": %lld, \"walk\": %lld, \"instance\": %lld}", ev_len, ev_walk, ev_inst);
  else std::printf("null");
  std::printf("}\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: orig_actions_host check|bfs|sim CFG ...\n"); return 2; }
  const std::string mode = argv[1];
  const OrigModel m = model_of(argv[2]);
  if (mode == "check") {
    long long mutations = 0;
    for (int a = 3; a < argc; ++a) {
      const std::string k = argv[a];
      if (k == "--mutations" && a + 1 < argc) mutations = std::atoll(argv[++a]);
      else if (k == "--seed" && a + 1 < argc) rng_state = std::strtoull(argv[++a], nullptr, 0);
      else { std::fprintf(stderr, "unknown argument %s\n", argv[a]); return 2; }
    }
    return main_check(m, mutations);
  }
  if (mode == "bfs") {
    bool inv_oom = true;
    for (int a = 3; a < argc; ++a) {
      if (!std::strcmp(argv[a], "--no-inv-oom")) inv_oom = false;
      else { std::fprintf(stderr, "unknown argument %s\n", argv[a]); return 2; }
    }
    return main_bfs(m, inv_oom);
  }
  if (mode == "sim") {
    const int rc = main_sim(m, argc, argv);
    if (rc == 2) std::fprintf(stderr, "usage: orig_actions_host sim CFG SEED NUM DEPTH BATCH [--walk W] [--no-inv-oom]\n");
    return rc;
  }
  std::fprintf(stderr, "unknown mode %s\n", mode.c_str());
  return 2;
}
