// TEST HARNESS ONLY (never part of the product).  A single-threaded host mirror of the GPU's
// simulation mode (raft-tla_amd/csrc/orig_sim.hip): the same successor function (orig_spec.h) and
// the same counter-based draws and selection rule (sim_rng.h), with a loop of its own -- every
// instance through S::apply, every successor's constraints and ALL the cfg's invariants evaluated
// (no ballots, no shortcuts, no frame condition), the in-model successors of a step collected
// first and the reservoir rule run over the list afterwards.
// Shape: -DSHAPE_N=.. -DSHAPE_NV=.. -DSHAPE_MT=.. -DSHAPE_ML=.. -DSHAPE_MK=..
//   orig_sim_host CFG SEED NUM DEPTH BATCH [--walk W] [--no-inv-oom] [--first W0]
// Without --walk: one JSON line {generated, actions{}, steps, walks, depth, event{length, walk,
// instance} | null, first_pick[]} for walks FIRST .. NUM-1 in batches of BATCH (the run stops
// after the first batch with an event; first_pick[k] = walks whose first step chose instance k).
// With --walk W: walk W alone, one canonical state per line (the violating state last, when the
// walk ends in a violation) -- the input of the oracle's check-trace.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../raft-tla_amd/csrc/orig_text.h"
#include "../../raft-tla_amd/csrc/sim_rng.h"

using namespace rmc;
using S = Orig<SHAPE_N, SHAPE_NV, SHAPE_MT, SHAPE_ML, SHAPE_MK>;
using W = S::Work;

struct Cand { int k, act; W t; };

struct Walk {
  std::vector<W> states;
  long long steps = 0;
  long long gen[OA_NACT] = {0};
  bool event = false;
  int ev_inst = -1;
  int first_pick = -1;
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
      if ((in || inv_oom) && viol < 0 && S::violated(c.t, m.rt.invariants)) { viol = k; viol_state = c.t; }
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
    if (step == 0) out.first_pick = inmodel[keep].k;
    cur = inmodel[keep].t;
    out.states.push_back(cur);
  }
  return out;
}

int main(int argc, char** argv) {
  if (argc < 6) { std::fprintf(stderr, "usage: orig_sim_host CFG SEED NUM DEPTH BATCH [--walk W] [--no-inv-oom] [--first W0]\n"); return 2; }
  CfgFile cfg = parse_cfg_text(read_text_file(argv[1]));
  OrigModel m = resolve_orig_model(cfg);
  const u64 seed = std::strtoull(argv[2], nullptr, 0);
  const long long num = std::atoll(argv[3]);
  int depth = std::atoi(argv[4]);
  if (depth <= 0) depth = (int)SIM_DEFAULT_DEPTH;
  long long batch = std::atoll(argv[5]);
  if (batch <= 0) batch = SIM_DEFAULT_BATCH;
  long long one = -1, first = 0;
  bool inv_oom = true;
  for (int a = 6; a < argc; ++a) {
    if (!std::strcmp(argv[a], "--walk") && a + 1 < argc) one = std::atoll(argv[++a]);
    else if (!std::strcmp(argv[a], "--first") && a + 1 < argc) first = std::atoll(argv[++a]);
    else if (!std::strcmp(argv[a], "--no-inv-oom")) inv_oom = false;
    else { std::fprintf(stderr, "unknown argument %s\n", argv[a]); return 2; }
  }
  if (one >= 0) {
    const Walk w = run_walk(m, inv_oom, seed, (u64)one, depth);
    for (const W& st : w.states) std::printf("%s\n", orig_state_text<S>(m, st, false).c_str());
    return 0;
  }
  long long generated = 0, steps = 0, walks = 0, longest = 1, gen[OA_NACT] = {0};
  std::vector<long long> first_pick(S::NI, 0);
  bool have = false;
  long long ev_len = 0, ev_walk = 0, ev_inst = 0;
  for (long long w0 = first; w0 < num && !have; w0 += batch) {
    const long long n = std::min(batch, num - w0);
    for (long long w = w0; w < w0 + n; ++w) {
      const Walk r = run_walk(m, inv_oom, seed, (u64)w, depth);
      steps += r.steps;
      for (int a = 0; a < OA_NACT; ++a) { gen[a] += r.gen[a]; generated += r.gen[a]; }
      longest = std::max<long long>(longest, (long long)r.states.size());
      if (r.first_pick >= 0) ++first_pick[r.first_pick];
      if (r.event) {
        const long long len = (long long)r.states.size();
        // minimum (length, walk, instance); walks ascend, so only a shorter trace replaces
        if (!have || len < ev_len) { ev_len = len; ev_walk = w; ev_inst = r.ev_inst; }
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
  std::printf(", \"first_pick\": [");
  for (int k = 0; k < S::NI; ++k) std::printf("%s%lld", k ? ", " : "", first_pick[k]);
  std::printf("]}\n");
  return 0;
}
