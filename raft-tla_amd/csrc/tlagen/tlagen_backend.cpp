// tlagen_backend.cpp — the generated path behind the C ABI (mc_opts.frontend, SURVEY.md §8(f)
// rank 3): a module + cfg outside the hand-compiled families (or any module, on request) is
// parsed by the SANY-subset front end, compiled to C++ over tlv.h together with the BFS kernels
// of tlagen_kernels.h, turned into a gfx950 code object by hiprtc (cached by source hash next
// to the library, or prebuilt by the build for the repo's own test specs), and run level by
// level from here.  The same module text gives the same counts as the hand-compiled kernels
// (tests/test_tlagen.py, tests/test_gpu_tlagen.py).
//
// Host structure (as OrigGpu / MembGpu): run_once() is set-up, a level loop over named steps and
// the report; what one search carries lives in a Search; launch() is the one place a kernel of
// the code object is queued; DevOwner owns every device buffer and event.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>

#include "../../../include/raftmc.h"
#include "../backend.h"
#include "../ckpt_file.h"
#include "../dev_owner.h"
#include "tla_gen.h"
#include "tlv_print.h"
#include "tlv_text.h"

namespace rmc {

// tlagen_sort.hip.  tmp == nullptr: *tmp_bytes = the temporary bytes the sort of n keys needs
int tlagen_sort_keys(const unsigned long long* keys_in, unsigned long long* keys_out, unsigned long long n, int bits,
                     void* tmp, size_t* tmp_bytes, hipStream_t s);
int tlagen_state_sizes(const unsigned int* words, unsigned long long used, const unsigned long long* offs, unsigned long long first,
                       unsigned long long n, int nv, unsigned long long* sizes, hipStream_t s);
int tlagen_pack_states(const unsigned int* words, const unsigned long long* offs, unsigned long long first, unsigned long long n,
                       const unsigned long long* at, unsigned int* out, hipStream_t s);

namespace {

using u32 = unsigned int;
using u64 = unsigned long long;

// counters of tlagen_kernels.h
enum { C_GEN = 0, C_GIN = 1, C_ERR = 2, C_CAP = 3, C_FLAG = 4, C_KIND = 5, C_SID = 6, C_INV = 7, C_EACT = 8, C_EWORDS = 9,
       C_EV = 10, C_EVINV = 11, C_NEWPOS = 12, C_ACT = 16 };

// The host mirror of the device's counters, by name: the fixed ones above, a generated and a
// distinct count per action from C_ACT on, and n_committed, n_states, words_used at the end.
struct Counters {
  std::vector<u64> h;
  int nact;
  explicit Counters(int nact_) : h(C_ACT + 2 * (size_t)nact_ + 4), nact(nact_) {}
  size_t bytes() const { return h.size() * 8; }
  size_t i_committed() const { return h.size() - 3; }
  size_t i_states() const { return h.size() - 2; }
  size_t i_words() const { return h.size() - 1; }
  size_t head_bytes() const { return i_committed() * 8; }   // all but the last three
  u64& operator[](size_t k) { return h[k]; }
  u64& n_committed() { return h[i_committed()]; }
  u64& n_states() { return h[i_states()]; }
  u64& words_used() { return h[i_words()]; }
  u64& act_generated(int k) { return h[C_ACT + k]; }
  u64& act_distinct(int k) { return h[C_ACT + nact + k]; }
};

struct KArgs {   // tlk::Args, field for field
  u32* words; u64* words_used; u64 words_cap;
  u64* offs; u64* parent; u32* act; u64 states_cap;
  u64* n_states; u64* n_committed;
  u64* table; u64 table_mask;
  u32* arena; u32 acap;
  u32* hstack; u32 hcap;
  u64* ctr;
  u32* evbuf; u32 evcap;
  u64 first, count;
  u64 seed;
  int inv_oom, deadlock;
  int fifo;
  u64* newpos; u64 newpos_cap;
  const u64* wkeys; u64 n_w;
  u64 level_end;
  u64 stop_rank, stop_ord;
  int stop_kind;
};

std::string read_all(const std::string& p) {
  std::ifstream f(p, std::ios::binary);
  if (!f) return "";
  std::stringstream ss; ss << f.rdbuf();
  return ss.str();
}
u64 fnv64(const std::string& s) {
  u64 h = 1469598103934665603ull;
  for (unsigned char ch : s) { h ^= ch; h *= 1099511628211ull; }
  return h;
}
std::string hex(u64 v) { char b[17]; std::snprintf(b, sizeof b, "%016llx", v); return b; }
std::string dir_of(const std::string& p) { const size_t s = p.rfind('/'); return s == std::string::npos ? "." : p.substr(0, s); }

std::string lib_dir() {
  Dl_info info;
  if (dladdr((void*)&lib_dir, &info) && info.dli_fname) return dir_of(info.dli_fname);
  return ".";
}

const char* kOpts[] = {"--offload-arch=gfx950", "-O2", "-std=c++17"};
// per-lane stack of a kernel that evaluates recursive function definitions (tlv::kMaxRecDepth
// nested calls of a few hundred bytes each, over the kernel's own frame)
constexpr size_t kRecStackBytes = 16384;
// the text the generator emits into a recursive function definition's depth guard: a source holding
// it gets kRecStackBytes per lane (scripts/check_isa.py reads the same marker)
constexpr const char* kRecMarker = "kMaxRecDepth) {";

#define HIPOK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { err = std::string(#x) + ": " + hipGetErrorString(e_); return MC_E_NO_DEVICE; } } while (0)

struct Meta {
  std::vector<std::string> vars, actions, invariants, atoms;
};

// the generated source names its variables, actions, invariants and atoms in "//@" lines
Meta parse_meta(const std::string& src) {
  Meta m;
  std::istringstream in(src);
  std::string line;
  while (std::getline(in, line)) {
    if (line.rfind("//@", 0) != 0) { if (!line.empty() && line[0] != '/') break; continue; }
    const size_t sp = line.find(' ');
    const std::string kind = line.substr(3, sp - 3), val = sp == std::string::npos ? "" : line.substr(sp + 1);
    if (kind == "var") m.vars.push_back(val);
    else if (kind == "action") m.actions.push_back(val);
    else if (kind == "invariant") m.invariants.push_back(val);
    else if (kind == "atom") m.atoms.push_back(val);
  }
  return m;
}

// One run's loaded code object: its kernels, and the stack limit a recursive module raised.  Loaded
// on every run and unloaded at its end.
struct Module {
  hipModule_t mod = nullptr;
  hipFunction_t init = nullptr, expand = nullptr, keys = nullptr, mat = nullptr, stop = nullptr, rebuild = nullptr;
  size_t prev_stack = 0;       // the device's stack limit before a recursive module raised it
  bool stack_raised = false;
  Module() = default; Module(const Module&) = delete; Module& operator=(const Module&) = delete;
  ~Module() {
    // hipLimitStackSize is process-wide: later kernels (the hand-compiled paths) get their limit back
    if (stack_raised) (void)hipDeviceSetLimit(hipLimitStackSize, prev_stack);
    if (mod) (void)hipModuleUnload(mod);
  }
  // A spec with a recursive function definition compiles to kernels whose stack size the
  // compiler cannot bound (dynamic stack): give each lane room for tlv::kMaxRecDepth nested
  // calls (the generated code refuses deeper recursion with an evaluation error), instead of the
  // runtime's default, which the static part of such a kernel's frame already exceeds.
  // (scripts/check_isa.py fails the build for a code object with a dynamic stack whose source lacks
  // the marker, or with a static frame above kRecStackBytes)
  int load(const std::string& image, bool recursive, bool recovering, std::string& err) {
    if (recursive) {
      HIPOK(hipDeviceGetLimit(&prev_stack, hipLimitStackSize));
      HIPOK(hipDeviceSetLimit(hipLimitStackSize, kRecStackBytes));
      stack_raised = true;
    }
    HIPOK(hipModuleLoadData(&mod, image.data()));
    HIPOK(hipModuleGetFunction(&init, mod, "tlg_init_k"));
    HIPOK(hipModuleGetFunction(&expand, mod, "tlg_expand_k"));
    HIPOK(hipModuleGetFunction(&keys, mod, "tlg_keys_k"));
    HIPOK(hipModuleGetFunction(&mat, mod, "tlg_mat_k"));
    HIPOK(hipModuleGetFunction(&stop, mod, "tlg_stop_k"));
    if (recovering) HIPOK(hipModuleGetFunction(&rebuild, mod, "tlg_rebuild_k"));
    return 0;
  }
};

// the bytes of the run's device buffers (0: none)
struct Sizes {
  u64 words, offs, parent, act, table, ctr, arena, hstack, ev, newpos, keys, sorted;
  bool operator==(const Sizes& x) const { return std::memcmp(this, &x, sizeof x) == 0; }
};

// What one run_once carries from step to step.
struct Search {
  const RunOpts& o;
  RunResult& r;
  std::string& err;
  // TLC -workers 1: the single-worker FIFO order (two passes per level, tlagen_kernels.h); any
  // other -workers: first-come insertion, every count TLC prints is order independent, and an
  // event is searched again in FIFO order for TLC's counterexample and stop point
  const bool fifo;
  // TLC -checkpoint / -recover: the levels' states every checkpoint_every levels
  // to checkpoint_path; the search continued from recover_path's
  const bool saving, recovering;
  // RAFTMC_TLAGEN_TIMING=1: where mc_run's wall time goes outside the kernels (stderr)
  const bool timing;
  const std::chrono::steady_clock::time_point t_start = std::chrono::steady_clock::now();
  double t_co = 0, t_setup = 0, t_load = 0;
  Module mod;
  KArgs a{};
  Counters c;
  u64 store = 0, words_cap = 0, lanes = 0, grid = 0;
  u64 first = 0, count = 0;         // the level being expanded
  u64 gen_prev = 0;
  u64 fifo_ev = ~0ull;              // FIFO: the stop point's event word
  // FIFO: the counters before the level (the stop point's report adds the level's part to them)
  std::vector<int64_t> prior_gen, prior_dist;
  int64_t prior_generated = 0;

  Search(const RunOpts& o_, RunResult& r_, std::string& err_, int nact)
      : o(o_), r(r_), err(err_), fifo(o_.workers == 1), saving(o_.checkpoint_every > 0 && !o_.checkpoint_path.empty()),
        recovering(!o_.recover_path.empty()), timing(std::getenv("RAFTMC_TLAGEN_TIMING") != nullptr), c(nact),
        prior_gen(nact, 0), prior_dist(nact, 0) {}
  double since() const { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count(); }
};

struct TlagenBackend : Backend {
  std::string src, key, src_origin;
  Meta meta;
  RunResult last;
  // The run's device buffers (store, seen-set, lane arenas, FIFO key arrays) and the timing event
  // pair, kept from one run to the next when the sizes and the device are unchanged: allocating a
  // 200 GiB store costs ~2.5 s on MI355X and freeing the buffers ~2.5 s more
  // (scripts/hipmalloc_time.py), i.e. a quarter of C2's run, so only a changed size (or a larger
  // arena after an overflow) allocates again.  The store stays readable after run() for
  // dump_states / traces.
  DevOwner<HipDevApi> res_;
  u32 *d_words_ = nullptr, *d_act_ = nullptr, *d_arena_ = nullptr, *d_hs_ = nullptr, *d_ev_ = nullptr;
  u64 *d_offs_ = nullptr, *d_parent_ = nullptr, *d_table_ = nullptr, *d_ctr_ = nullptr, *d_newpos_ = nullptr, *d_keys_ = nullptr,
      *d_sorted_ = nullptr;
  hipEvent_t e0_ = nullptr, e1_ = nullptr;
  void* d_sort_tmp_ = nullptr;      // the radix sort's temporary buffer: lives for one run
  size_t sort_tmp_bytes_ = 0;
  Sizes alloc_{};
  int alloc_dev_ = -1;
  u64 n_stored = 0, words_stored = 0;
  bool store_complete = true;   // false after a store overflow (ids handed out without words)
  int dev = 0;
  u32 arena_scale = 1;
  bool arena_overflow = false;
  std::string workers_event_;   // what a -workers N search stopped on (named if its FIFO re-search overflows)

  TlagenBackend(const std::string& tla_path, const CfgFile& cfg) {
    if (tla_path.size() > 8 && tla_path.compare(tla_path.size() - 8, 8, ".gen.hip") == 0) {
      src = read_all(tla_path);
      if (src.empty()) throw CfgError(MC_E_IO, "cannot read " + tla_path);
      src_origin = "pregenerated " + tla_path;
    } else {
      std::vector<std::string> dirs;
      if (const char* e = std::getenv("RAFTMC_TLA_PATH")) {
        std::string s = e;
        size_t a = 0;
        while (a <= s.size()) { size_t b = s.find(':', a); if (b == std::string::npos) b = s.size(); if (b > a) dirs.push_back(s.substr(a, b - a)); a = b + 1; }
      }
      tlagen::Program prog;
      try { prog = tlagen::load_program(tla_path, dirs); }
      catch (const tlagen::ParseError& e) { throw CfgError(MC_E_PARSE, e.what()); }
      tlagen::Generated g = tlagen::generate(prog, cfg);
      src = tlagen::compose_source(g, kTlvText, kTlgKernelsText);
      src_origin = "front end: " + tla_path;
    }
    meta = parse_meta(src);
    if (meta.vars.empty()) throw CfgError(MC_E_PARSE, "generated source without metadata");
    std::string k = src;
    for (const char* o : kOpts) k += std::string("\n") + o;
    key = hex(fnv64(k));
  }
  ~TlagenBackend() override { release(); }
  void release_device() override { release(); }
  void release() {
    res_.release();
    alloc_ = Sizes{}; alloc_dev_ = -1; sort_tmp_bytes_ = 0;
  }

  std::string family() const override { return "tlagen"; }
  std::string describe_json() const override {
    std::string o = "{\"family\": \"tlagen\", \"origin\": \"" + src_origin + "\", \"code_object\": \"" + key + "\", \"variables\": [";
    for (size_t i = 0; i < meta.vars.size(); ++i) o += (i ? ", \"" : "\"") + meta.vars[i] + "\"";
    o += "], \"actions\": [";
    for (size_t i = 0; i < meta.actions.size(); ++i) o += (i ? ", \"" : "\"") + meta.actions[i] + "\"";
    return o + "]}";
  }
  int nact() const { return (int)meta.actions.size(); }
  std::string action_name(u64 k) const { return k < meta.actions.size() ? meta.actions[k] : "?"; }
  std::string inv_name(u64 i) const { return i < meta.invariants.size() ? meta.invariants[i] : std::string("?"); }
  // TLA+ text of a state's canonical words (tlv_print.h); join: "\n" for traces, " " for dumps
  std::string state_text(const u32* w, const char* join) const {
    return tlvprint::printer([this](u32 i) { return i < meta.atoms.size() ? meta.atoms[i].c_str() : nullptr; },
                             [this](size_t i) { return meta.vars[i].c_str(); }, meta.vars.size()).state(w, join);
  }

  // code object: cache file, else hiprtc
  int code_object(std::string& image, std::string& err) {
    std::vector<std::string> dirs;
    if (const char* e = std::getenv("RAFTMC_TLAGEN_CACHE")) dirs.push_back(e);
    dirs.push_back(lib_dir() + "/tlagen_co");
    for (auto& d : dirs) {
      image = read_all(d + "/" + key + ".hsaco");
      if (!image.empty()) return 0;
    }
    hiprtcProgram prog;
    if (hiprtcCreateProgram(&prog, src.c_str(), "tlagen.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS) { err = "hiprtcCreateProgram failed"; return MC_E_NO_DEVICE; }
    const hiprtcResult rc = hiprtcCompileProgram(prog, 3, kOpts);
    if (rc != HIPRTC_SUCCESS) {
      size_t n = 0; hiprtcGetProgramLogSize(prog, &n);
      std::string log(n, '\0'); if (n) hiprtcGetProgramLog(prog, &log[0]);
      hiprtcDestroyProgram(&prog);
      err = "hiprtc: " + log.substr(0, 4000);
      return MC_E_UNSUPPORTED;
    }
    size_t n = 0; hiprtcGetCodeSize(prog, &n);
    image.assign(n, '\0'); hiprtcGetCode(prog, &image[0]);
    hiprtcDestroyProgram(&prog);
    for (auto& d : dirs) {   // best effort: keep it for the next open (written aside, then renamed)
      ::mkdir(d.c_str(), 0755);
      const std::string path = d + "/" + key + ".hsaco", tmp = path + ".tmp" + std::to_string((long)::getpid());
      std::ofstream f(tmp, std::ios::binary);
      if (!f) continue;
      f.write(image.data(), (std::streamsize)image.size());
      f.close();
      if (f && std::rename(tmp.c_str(), path.c_str()) == 0) break;
      std::remove(tmp.c_str());
    }
    return 0;
  }

  int run(const RunOpts& o, RunResult& r, std::string& err) override {
    // a lane arena too small for one state's successors: searched again with 4x the arena per lane
    // on a quarter of the lanes (the same HBM), up to 64x (C2: 16K words; the Apalache spec's
    // states are ~1.4K words and need more)
    for (arena_scale = 1;; arena_scale *= 4) {
      bool again = false;
      int rc = run_once(o, r, err, again);
      if (rc == 0 && again) {
        // TLC -workers N found an event: TLC's counterexample and stop point are the single-worker
        // search's, so the model is searched again in FIFO order (as the hand-compiled paths do).
        // That search needs more HBM per state (44 B of bookkeeping instead of 20, 16-B seen-set
        // entries): when it does not fit, the event the first search found is still reported
        RunOpts o1 = o;
        o1.workers = 1;
        o1.recover_path.clear();      // a checkpoint of this search is in its order, not TLC's: start over
        o1.checkpoint_path.clear();
        const std::string found = workers_event_;
        rc = run_once(o1, r, err, again);
        if (rc == 0 && r.verdict == MC_VERDICT_CAPACITY_OVERFLOW && !arena_overflow)
          r.error = "the -workers N search found " + found + "; TLC's single-worker re-search of it (for TLC's "
                    "counterexample and stop point) ran out of capacity: " + r.error;
      }
      if (rc != 0 || !arena_overflow || arena_scale >= 64) return rc;
    }
  }

  // one search in one order with one arena size: set-up, the level loop, the report
  int run_once(const RunOpts& o, RunResult& r, std::string& err, bool& again) {
    again = false;
    arena_overflow = false;
    Search s(o, r, err, nact());
    struct SortTmp {   // freed on every return (the other device buffers stay)
      TlagenBackend& b;
      ~SortTmp() { b.res_.free(&b.d_sort_tmp_); b.sort_tmp_bytes_ = 0; }
    } sort_tmp{*this};
    if (int rc = begin_search(s)) return rc;
    if (int rc = seed_init(s)) return rc;
    while (s.count && !s.c[C_FLAG] && !s.c[C_CAP]) {
      if (o.max_depth && r.depth >= o.max_depth) { r.verdict = MC_VERDICT_DEPTH_LIMIT; r.left_on_queue = (int64_t)s.count; break; }
      s.a.first = s.first; s.a.count = s.count;
      r.levels.push_back({0, 0, 0});
      u64 fresh = 0;
      bool complete = true;
      if (int rc = s.fifo ? fifo_level(s, fresh, complete) : expand_level(s, fresh)) return rc;
      // the level is not complete at a stop: only completed levels are reported (as TLC does)
      if (!complete) { r.levels.pop_back(); break; }
      if (int rc = commit_level(s, fresh)) return rc;
    }
    return report(s, again);
  }

  // Every kernel of the code object is queued here, on the null stream, and waited for: the event
  // pair's time goes to the run and to the current level, and the counters come back to the mirror.
  // Every kernel but tlg_keys_k takes the Args block (tlk::Args).
  int launch(Search& s, hipFunction_t f, u64 blocks, unsigned bs, void** own_params = nullptr) {
    std::string& err = s.err;
    void* args[] = {&s.a};
    void** params = own_params ? own_params : args;
    HIPOK(hipEventRecord(e0_, 0));
    HIPOK(hipModuleLaunchKernel(f, (unsigned)blocks, 1, 1, bs, 1, 1, 0, 0, params, nullptr));
    HIPOK(hipEventRecord(e1_, 0));
    HIPOK(hipEventSynchronize(e1_));
    float ms = 0; (void)hipEventElapsedTime(&ms, e0_, e1_);
    s.r.seconds_kernels += ms / 1e3;
    s.r.levels.empty() ? void() : void(s.r.levels.back().kernel_ms += ms);
    HIPOK(hipMemcpy(s.c.h.data(), d_ctr_, s.c.bytes(), hipMemcpyDeviceToHost));
    return 0;
  }
  int set_ctr(Search& s, size_t k, u64 v) {
    std::string& err = s.err;
    HIPOK(hipMemcpy(d_ctr_ + k, &v, 8, hipMemcpyHostToDevice));
    return 0;
  }

  // the buffers of these sizes and the event pair on device d: kept when nothing changed, else all
  // released and created again (a failed allocation keeps nothing)
  int ensure_alloc(int d, const Sizes& want, std::string& err) {
    if (d == alloc_dev_ && want == alloc_) return 0;
    release();
    auto buf = [&](auto** p, u64 bytes) { return !bytes || res_.device(p, bytes) == hipSuccess; };
    if (!(buf(&d_words_, want.words) && buf(&d_offs_, want.offs) && buf(&d_parent_, want.parent) && buf(&d_act_, want.act) &&
          buf(&d_table_, want.table) && buf(&d_ctr_, want.ctr) && buf(&d_arena_, want.arena) && buf(&d_hs_, want.hstack) &&
          buf(&d_ev_, want.ev) && buf(&d_newpos_, want.newpos) && buf(&d_keys_, want.keys) && buf(&d_sorted_, want.sorted))) {
      release();
      err = "device allocation failed";
      return MC_E_OOM;
    }
    if (res_.event(&e0_) != hipSuccess || res_.event(&e1_) != hipSuccess) {
      release();
      err = "hipEventCreate failed";
      return MC_E_NO_DEVICE;
    }
    alloc_ = want; alloc_dev_ = d;
    return 0;
  }

  // option refusal, the code object and its module, then the device side
  int begin_search(Search& s) {
    std::string& err = s.err;
    if (!s.o.disjunct_copies) {   // the generated code enumerates disjuncts as TLC does (MC_COMPAT_DISJUNCT_COPIES)
      err = "the generated path counts TLC's disjunct copies; MC_COMPAT_DISJUNCT_COPIES cannot be cleared on it";
      return MC_E_UNSUPPORTED;
    }
    dev = s.o.device;
    HIPOK(hipSetDevice(dev));
    std::string image;
    if (int rc = code_object(image, err)) return rc;
    s.t_co = s.since();
    if (int rc = s.mod.load(image, src.find(kRecMarker) != std::string::npos, s.recovering, err)) return rc;
    return lay_out(s);
  }

  // HBM layout: store words + per-state offsets/parents/actions, seen-set, lanes' arenas (+ FIFO:
  // the level's inserted entries and their keys, unsorted and sorted); allocation, clears, KArgs
  int lay_out(Search& s) {
    std::string& err = s.err;
    const RunOpts& o = s.o;
    s.store = o.state_store_bytes ? o.state_store_bytes : (16ull << 30);
    // canonical words dominate (C2: ~350-450 words per state); 20 B per state for offsets, parents,
    // actions (+ 24 B of per-level key arrays in FIFO order)
    const u64 per_state = s.fifo ? 44 : 20;
    const u64 states_cap = s.store / 7 / per_state;
    s.words_cap = (s.store - states_cap * per_state) / 4;
    const u64 entry = s.fifo ? 16 : 8;
    const u64 tbytes = o.fp_table_bytes ? o.fp_table_bytes : (2ull << 30);
    u64 slots = 1; while (slots * 2 * entry <= tbytes) slots *= 2;
    const u32 acap = 16384 * arena_scale, hcap = 4096 * arena_scale, evcap = 65536 * arena_scale;
    int ncu = 256;
    (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
    int waves = 8;   // per CU: 2 per SIMD (the expand kernel holds ~250 VGPRs)
    if (const char* e = std::getenv("RAFTMC_TLAGEN_WAVES")) waves = std::max(1, std::atoi(e));
    s.lanes = std::max<u64>(64, (u64)ncu * waves * 64 / arena_scale);
    s.grid = s.lanes / 64;
    const u64 kcap = s.fifo ? std::min<u64>(states_cap, slots) : 1;
    const u64 kb = s.fifo ? kcap * 8 : 0;
    if (int rc = ensure_alloc(dev, {s.words_cap * 4, states_cap * 8, states_cap * 8, states_cap * 4, slots * entry, s.c.bytes(),
                                    s.lanes * acap * 4, s.lanes * hcap * 4, (u64)evcap * 4, kb, kb, kb}, err)) return rc;
    n_stored = 0; words_stored = 0; store_complete = false;
    HIPOK(hipMemset(d_table_, 0, slots * entry));
    HIPOK(hipMemset(d_ctr_, 0, s.c.bytes()));
    if (s.timing) HIPOK(hipDeviceSynchronize());
    s.t_setup = s.since();
    KArgs& a = s.a;
    a.words = d_words_; a.words_used = d_ctr_ + s.c.i_words(); a.words_cap = s.words_cap;
    a.offs = d_offs_; a.parent = d_parent_; a.act = d_act_; a.states_cap = states_cap;
    a.n_states = d_ctr_ + s.c.i_states();
    a.n_committed = d_ctr_ + s.c.i_committed();
    a.table = d_table_; a.table_mask = slots - 1;
    a.arena = d_arena_; a.acap = acap; a.hstack = d_hs_; a.hcap = hcap;
    a.ctr = d_ctr_; a.evbuf = d_ev_; a.evcap = evcap;
    a.seed = o.seed ? o.seed : 0x2545f4914f6cdd1dull;
    a.inv_oom = o.inv_out_of_model ? 1 : 0;
    a.deadlock = o.check_deadlock ? 1 : 0;
    a.fifo = s.fifo ? 1 : 0;
    a.newpos = d_newpos_; a.newpos_cap = kcap;
    s.r = RunResult();
    s.r.action_names = meta.actions;
    return 0;
  }

  // the first level: Init's states, or a checkpoint's
  int seed_init(Search& s) {
    RunResult& r = s.r;
    if (!s.recovering) {
      if (int rc = launch(s, s.mod.init, 1, 64)) return rc;
      s.count = s.c.n_states();
      r.generated = (int64_t)s.c[C_GEN];
      if (s.count) { r.depth = 1; r.levels.push_back({(int64_t)s.count, (int64_t)s.c[C_GEN], 0}); }
    } else {
      // the file's states, counters and BFS position instead of Init; then the seen-set from the
      // states.  The restored levels come after the rebuild: its time is the run's, not a level's
      std::vector<LevelStat> levels;
      if (int rc = load_checkpoint(s, levels)) return rc;
      s.t_load = s.since() - s.t_setup;
      if (!s.c[C_CAP]) {
        s.a.first = 0; s.a.count = s.c.n_states();
        if (int rc = launch(s, s.mod.rebuild, s.grid, 64)) return rc;
        if (s.c[C_ERR]) return ckpt::Reader(s.o.recover_path).other_model(s.err);   // a stored state is none of this model's
      }
      r.levels = levels;
    }
    s.gen_prev = s.c[C_GEN];
    return 0;
  }

  // a -workers N level: one pass, first-come insertion
  int expand_level(Search& s, u64& fresh) {
    if (int rc = launch(s, s.mod.expand, s.grid, 64)) return rc;
    fresh = s.c.n_states() - (s.first + s.count);
    return 0;
  }

  // a FIFO level: pass 1 puts the successors' keys into the seen-set, the new entries' keys are
  // sorted, pass 2 stores the winners in key order.  complete = false: the level ended in an
  // overflow or in an event (fifo_ev)
  int fifo_level(Search& s, u64& fresh, bool& complete) {
    KArgs& a = s.a;
    complete = false;
    s.prior_generated = (int64_t)s.c[C_GEN];
    for (int k = 0; k < nact(); ++k) { s.prior_gen[k] = (int64_t)s.c.act_generated(k); s.prior_dist[k] = (int64_t)s.c.act_distinct(k); }
    if (set_ctr(s, C_EV, ~0ull) || set_ctr(s, C_NEWPOS, 0)) return MC_E_NO_DEVICE;
    const u64 level_end = s.first + s.count;
    a.wkeys = nullptr; a.n_w = 0; a.level_end = level_end;
    if (int rc = launch(s, s.mod.expand, s.grid, 64)) return rc;   // pass 1: keys into the seen-set
    if (s.c[C_CAP]) return 0;
    const u64 nw = s.c[C_NEWPOS];
    if (nw) {
      {   // tlg_keys_k(table, newpos, n, keys)
        const u64* kt = d_table_; const u64* kn = d_newpos_; u64 kcount = nw; u64* kk = d_keys_;
        void* kp[] = {(void*)&kt, (void*)&kn, (void*)&kcount, (void*)&kk};
        if (int rc = launch(s, s.mod.keys, std::min<u64>(4096, (nw + 255) / 256), 256, kp)) return rc;
      }
      if (sort_keys(nw)) { s.err = "radix sort of the level's keys failed"; return MC_E_NO_DEVICE; }
      a.wkeys = d_sorted_; a.n_w = nw; a.level_end = level_end;
      if (int rc = launch(s, s.mod.mat, s.grid, 64)) return rc;     // pass 2: the winners, in key order
      const u64 total = level_end + nw;
      if (hipMemcpy(d_ctr_ + s.c.i_states(), &total, 8, hipMemcpyHostToDevice) != hipSuccess) { s.err = "counter write failed"; return MC_E_NO_DEVICE; }
      s.c.n_states() = total;
    }
    fresh = nw;
    if (s.c[C_CAP]) return 0;
    if (s.c[C_EV] != ~0ull) { s.fifo_ev = s.c[C_EV]; return 0; }
    complete = true;
    return 0;
  }
  // d_keys_[0, n) -> d_sorted_, ascending; the temporary buffer grows as needed
  int sort_keys(u64 n) {
    size_t need = 0;
    if (tlagen_sort_keys(d_keys_, d_sorted_, n, 64, nullptr, &need, 0)) return -1;
    if (need > sort_tmp_bytes_) {
      sort_tmp_bytes_ = 0;
      if (res_.device(&d_sort_tmp_, need) != hipSuccess) return -2;
      sort_tmp_bytes_ = need;
    }
    return tlagen_sort_keys(d_keys_, d_sorted_, n, 64, d_sort_tmp_, &sort_tmp_bytes_, 0);
  }

  // a completed level: its statistics, the next level's range, and the checkpoint rule
  int commit_level(Search& s, u64 fresh) {
    RunResult& r = s.r;
    ++r.n_launches;
    r.levels.back().states = (int64_t)fresh;
    r.levels.back().generated = (int64_t)(s.c[C_GEN] - s.gen_prev);
    s.gen_prev = s.c[C_GEN];
    s.first += s.count; s.count = fresh;
    if (fresh) ++r.depth; else r.levels.pop_back();
    // a completed, non-empty level; never after an overflow (the last good file stays) nor with a
    // -workers N event claimed (its level is cut short)
    if (s.saving && fresh && !s.c[C_CAP] && !s.c[C_FLAG] && r.depth % s.o.checkpoint_every == 0) return save_checkpoint(s);
    return 0;
  }

  // how the search ended: a -workers N event (searched again in FIFO order by run()), a capacity
  // overflow, the FIFO stop point, an event among the initial states, or no event at all
  int report(Search& s, bool& again) {
    RunResult& r = s.r;
    Counters& c = s.c;
    const double t_loop = s.since();
    if (s.timing && s.recovering)
      std::fprintf(stderr, "tlagen timing: recover read + upload %.3f s, %llu states, %llu words\n", s.t_load, c.n_states(), c.words_used());
    if (s.timing)
      std::fprintf(stderr, "tlagen timing: code object %.3f s, module load + allocation + clears %.3f s, level loop %.3f s "
                           "(kernels %.3f s), store %.1f GiB, arena %.1f GiB\n", s.t_co, s.t_setup - s.t_co, t_loop - s.t_setup,
                   r.seconds_kernels, s.store / 1073741824.0, (double)s.lanes * (s.a.acap + s.a.hcap) * 4 / 1073741824.0);
    if (!s.fifo && c[C_FLAG] && !c[C_CAP]) {
      // tlagen_kernels.h C_KIND: 1/2 violation, 3 evaluation error, 4 deadlock, 5 invariant evaluation error
      static const char* const kinds[] = {"an event", "an invariant violation", "an invariant violation",
                                          "an evaluation error", "a deadlock", "an invariant evaluation error"};
      const u64 kd = c[C_KIND];
      workers_event_ = std::string(kd < 6 ? kinds[kd] : "an event") + " at depth " + std::to_string(r.depth + 1);
      again = true;
      return 0;
    }
    // on a store overflow some ids were handed out without their words: only the committed states
    // are stored (and ids are no longer dense, so traces and dumps are refused below)
    store_complete = c.n_committed() == c.n_states();
    n_stored = store_complete ? c.n_states() : c.n_committed();
    words_stored = std::min<u64>(c.words_used(), s.words_cap);
    r.generated = (int64_t)c[C_GEN];
    r.generated_in_model = (int64_t)c[C_GIN];
    r.distinct = (int64_t)n_stored;
    r.act_generated.resize(nact()); r.act_distinct.resize(nact());
    for (int k = 0; k < nact(); ++k) { r.act_generated[k] = (int64_t)c.act_generated(k); r.act_distinct[k] = (int64_t)c.act_distinct(k); }
    if (c[C_CAP]) {
      arena_overflow = (c[C_CAP] & 4) != 0;
      r.verdict = MC_VERDICT_CAPACITY_OVERFLOW;
      r.error = (c[C_CAP] & 4) ? "lane arena too small for one state's successors" : (c[C_CAP] & 2) ? "seen-set full"
              : (c[C_CAP] & 8) ? "a state has more than 2^24 successors" : "state store full";
    } else if (s.fifo_ev != ~0ull) {
      if (int rc = fifo_stop(s)) return rc;
    } else if (c[C_FLAG]) {
      init_event(s);
    }
    r.seed = s.a.seed;
    r.state_bytes = 0;
    r.seconds_total = s.since();
    last = r;
    return 0;
  }

  // an event among the initial states (one lane, Init's order: TLC's)
  void init_event(Search& s) {
    RunResult& r = s.r;
    Counters& c = s.c;
    const u64 kind = c[C_KIND];
    trace_to(c[C_SID], r);
    if (kind == 1 || kind == 2) {
      r.verdict = MC_VERDICT_INVARIANT_VIOLATION;
      r.violated = inv_name(c[C_INV]);
      if (kind == 2) event_successor(s);   // the violating successor is outside the constraints: printed from the event buffer
    } else if (kind == 3) {
      r.verdict = MC_VERDICT_EVAL_ERROR;
      r.error = "evaluation error (tlv error bits " + std::to_string(c[C_INV]) + ") while computing the initial states";
    } else if (kind == 5) {   // TLC: "Evaluating invariant X failed." with the behavior up to the state
      r.verdict = MC_VERDICT_EVAL_ERROR;
      r.violated = inv_name(c[C_INV]);
      r.error = "Evaluating invariant " + r.violated + " failed.";
    } else {
      r.verdict = MC_VERDICT_DEADLOCK;
    }
    r.left_on_queue = (int64_t)s.count;
  }
  // the trace's last step from the event buffer: a successor that is no stored state
  void event_successor(Search& s) {
    std::vector<u32> w(s.c[C_EWORDS]);
    (void)hipMemcpy(w.data(), d_ev_, w.size() * 4, hipMemcpyDeviceToHost);
    s.r.trace.push_back({action_name(s.c[C_EACT]), state_text(w.data(), "\n")});
  }

  // TLC's report at the FIFO stop point: the level's first event in key order (tlagen_kernels.h
  // C_EV), its counters (generated = successor lists of the parents up to the event's; distinct =
  // the new states before it in key order, the violating one included; left on queue = the rest of
  // the level's parents plus the new states so far) and the counterexample
  int fifo_stop(Search& s) {
    std::string& err = s.err;
    RunResult& r = s.r;
    KArgs& a = s.a;
    Counters& c = s.c;
    const u64 key = s.fifo_ev >> 3, kind = s.fifo_ev & 7, rank = key >> 24, ord = key & ((1ull << 24) - 1);
    const u64 level_end = s.first + s.count, nw = a.n_w;
    const bool new_state = kind == 3 || kind == 5;   // EV_INV_ERROR_NEW / EV_VIOLATION_NEW
    // the winners before the event in key order (binary search over the sorted keys)
    u64 lo = 0, hi = a.wkeys ? nw : 0;
    while (lo < hi) {
      const u64 mid = (lo + hi) / 2;
      u64 kk = 0;
      HIPOK(hipMemcpy(&kk, a.wkeys + mid, 8, hipMemcpyDeviceToHost));
      if (kk < key || (kk == key && new_state)) lo = mid + 1; else hi = mid;
    }
    const u64 before = lo;
    // generated counts: re-derived over the parents [0, rank] (and the event successor captured)
    c[C_GEN] = 0;
    for (int k = 0; k < nact(); ++k) c.act_generated(k) = 0;
    HIPOK(hipMemcpy(a.ctr, c.h.data(), c.head_bytes(), hipMemcpyHostToDevice));
    a.stop_rank = rank; a.stop_ord = ord; a.stop_kind = (int)kind;
    if (int rc = launch(s, s.mod.stop, std::min<u64>(s.grid, (rank + 64) / 64), 64)) return rc;
    r.generated = s.prior_generated + (int64_t)c[C_GEN];
    for (int k = 0; k < nact(); ++k) r.act_generated[k] = s.prior_gen[k] + (int64_t)c.act_generated(k);
    std::vector<u32> acts(before);
    if (before) HIPOK(hipMemcpy(acts.data(), a.act + level_end, before * 4, hipMemcpyDeviceToHost));
    for (int k = 0; k < nact(); ++k) r.act_distinct[k] = s.prior_dist[k];
    for (u32 x : acts) if (x < (u32)nact()) ++r.act_distinct[x];
    r.distinct = (int64_t)(level_end + before);
    r.left_on_queue = (int64_t)(s.count - rank - 1 + before);
    n_stored = level_end + before;
    // tlagen_kernels.h's events: 0 EV_NEXT_ERROR, 1 EV_DEADLOCK, 2 EV_INV_ERROR_OOM (a constraint / VIEW /
    // invariant could not be evaluated on a successor), 3 EV_INV_ERROR_NEW, 4 EV_VIOLATION_OOM, 5 EV_VIOLATION_NEW
    r.verdict = kind == 1 ? MC_VERDICT_DEADLOCK : kind <= 3 ? MC_VERDICT_EVAL_ERROR : MC_VERDICT_INVARIANT_VIOLATION;
    if (kind >= 2) { r.violated = inv_name(c[C_EVINV]); r.depth += 1; }   // the event lies on a successor
    if (kind == 0) r.error = "evaluation error while computing the successors of the last state";
    if (kind == 2) r.error = "evaluation error on a successor of the last state (a constraint, the VIEW or invariant " + r.violated + ")";
    if (kind == 3) r.error = "Evaluating invariant " + r.violated + " failed.";
    // the counterexample ends in the new state itself, or in the event's parent and, for a successor
    // outside the model, what tlg_stop_k captured of it
    trace_to(kind == 3 || kind >= 5 ? level_end + before - 1 : s.first + rank, r);
    if (kind == 2 || kind == 4) {
      if (c[C_EWORDS]) event_successor(s);
      else err = "the stop point's successor was not re-derived";
    }
    return 0;
  }

  // ---------------------------------------------------------------- checkpoint / recover
  // ckpt::GenHead around the shared framing (ckpt_file.h).  What names the model in the file: the
  // code object's key (the generated source and its compile options, so every constant of the cfg)
  // and the variable and action names; not where the module lay.
  std::string ckpt_desc() const {
    std::string d = "tlagen " + key + " variables";
    for (auto& v : meta.vars) d += " " + v;
    d += " actions";
    for (auto& x : meta.actions) d += " " + x;
    return d;
  }
  static constexpr u64 kCkptChunkBytes = 256ull << 20;   // host staging of a save or a load

  // The store after a completed level.  The states' words go out packed in id order (tlagen_sort.hip);
  // the lanes' arenas and handle stacks, idle between levels, are the device staging, so a save
  // allocates nothing on the device and stages kCkptChunkBytes on the host whatever the store holds.
  int save_checkpoint(Search& s) {
    const KArgs& a = s.a;
    Counters& c = s.c;
    const RunResult& r = s.r;
    const int nv = (int)meta.vars.size();
    const u64 total = c.n_states(), used = c.words_used();
    const std::string desc = ckpt_desc();
    ckpt::GenHead g;
    std::memset(&g, 0, sizeof g);
    std::memcpy(g.magic, "RAFTMCG1", 8);
    g.nwp = 0; g.total = total; g.level_begin = s.first; g.level_count = s.count; g.seed = a.seed;
    g.words = used; g.fifo = s.fifo ? 1 : 0;
    g.generated = (int64_t)c[C_GEN]; g.distinct = (int64_t)total; g.depth = r.depth; g.generated_in_model = (int64_t)c[C_GIN];
    g.n_act = nact(); g.n_levels = (int64_t)r.levels.size(); g.desc_len = (int64_t)desc.size();
    std::vector<int64_t> act_generated(nact()), act_distinct(nact());
    for (int k = 0; k < nact(); ++k) { act_generated[k] = (int64_t)c.act_generated(k); act_distinct[k] = (int64_t)c.act_distinct(k); }
    u64* d_at = (u64*)a.hstack;                                                   // sizes, then offsets, of a chunk of states
    const u64 at_cap = std::min<u64>(1u << 20, s.lanes * a.hcap / 2 - 1);          // states per chunk
    const u64 stage_words = std::min<u64>(s.lanes * a.acap, kCkptChunkBytes / 4);  // packed words per chunk (>= a state: it fits a lane's arena)
    std::string why;
    auto body = [&](FILE* f) -> bool {
      std::vector<u64> buf(std::max<u64>(std::min(at_cap, total) + 1, std::min<u64>(kCkptChunkBytes / 8, std::max<u64>(total, (used + 1) / 2))));
      auto sizes = [&](u64 i0, u64 n) -> bool {   // buf[0, n) = words of the states [i0, i0 + n)
        if (tlagen_state_sizes(a.words, used, a.offs, i0, n, nv, d_at, 0) ||
            hipMemcpy(buf.data(), d_at, n * 8, hipMemcpyDeviceToHost) != hipSuccess) { why = "reading the store failed"; return false; }
        for (u64 k = 0; k < n; ++k) if (buf[k] == 0 || buf[k] > stage_words) { why = "a stored state is malformed"; return false; }
        return true;
      };
      u64 at = 0;   // offs: where each state begins in the packed words
      for (u64 i0 = 0; i0 < total; i0 += at_cap) {
        const u64 n = std::min(at_cap, total - i0);
        if (!sizes(i0, n)) return false;
        for (u64 k = 0; k < n; ++k) { const u64 sz = buf[k]; buf[k] = at; at += sz; }
        if (std::fwrite(buf.data(), 8, n, f) != n) return false;
      }
      if (at != used) { why = "the stored states do not add up to the stored words"; return false; }
      for (int kind = 1; kind <= 2; ++kind) {   // parent, act
        const size_t esz = kind == 1 ? 8 : 4;
        const u64 per = kCkptChunkBytes / esz;
        for (u64 i0 = 0; i0 < total; i0 += per) {
          const u64 n = std::min(per, total - i0);
          const void* from = kind == 1 ? (const void*)(a.parent + i0) : (const void*)(a.act + i0);
          if (hipMemcpy(buf.data(), from, n * esz, hipMemcpyDeviceToHost) != hipSuccess) { why = "reading the store failed"; return false; }
          if (std::fwrite(buf.data(), esz, n, f) != n) return false;
        }
      }
      for (u64 i0 = 0; i0 < total;) {   // words: as many states as the staging holds at a time
        const u64 n = std::min(at_cap, total - i0);
        if (!sizes(i0, n)) return false;
        u64 take = 0, w = 0;
        for (; take < n && w + buf[take] <= stage_words; ++take) { const u64 sz = buf[take]; buf[take] = w; w += sz; }
        buf[take] = w;
        if (hipMemcpy(d_at, buf.data(), (take + 1) * 8, hipMemcpyHostToDevice) != hipSuccess ||
            tlagen_pack_states(a.words, a.offs, i0, take, d_at, a.arena, 0) ||
            hipMemcpy(buf.data(), a.arena, w * 4, hipMemcpyDeviceToHost) != hipSuccess) { why = "reading the store failed"; return false; }
        if (std::fwrite(buf.data(), 4, w, f) != w) return false;
        i0 += take;
      }
      return true;
    };
    const int rc = ckpt::write_file(s.o.checkpoint_path, g, desc, act_generated, act_distinct, r.levels, body, s.err);
    if (rc && !why.empty()) s.err += " (" + why + ")";
    return rc;
  }

  // The file into the store and the counters (the mirror, and the device's); s.first / s.count: the
  // level the search goes on with.  A file that does not fit this run's store sets C_CAP in the
  // mirror alone and loads nothing: the run ends as a capacity overflow, as a search that outgrew
  // the store does.
  int load_checkpoint(Search& s, std::vector<LevelStat>& levels) {
    std::string& err = s.err;
    KArgs& a = s.a;
    Counters& c = s.c;
    const std::string& path = s.o.recover_path;
    ckpt::GenHead g;
    ckpt::Reader in(path);
    std::vector<int64_t> act_generated, act_distinct;
    if (int rc = in.head("RAFTMCG1", 0, nact(), ckpt_desc(), g, act_generated, act_distinct, levels, err)) return rc;
    if (int rc = ckpt::check_gen_head(in, g, levels, err)) return rc;
    if (s.fifo && !g.fifo) {
      err = "checkpoint " + path + " was written by a -workers N search: its kept parents are not TLC's single-worker "
            "FIFO ones, so it cannot resume a -workers 1 search";
      return MC_E_INVALID;
    }
    s.r.depth = g.depth;
    s.first = g.level_begin; s.count = g.level_count;
    a.seed = g.seed;
    if (g.total > a.states_cap || g.words > a.words_cap) { c[C_CAP] = 1; return 0; }
    auto upload = [&](int kind, const void* data, uint64_t i0, uint64_t n, std::string& e) -> int {
      void* dst = kind == 0 ? (void*)(a.offs + i0) : kind == 1 ? (void*)(a.parent + i0) : kind == 2 ? (void*)(a.act + i0) : (void*)(a.words + i0);
      if (hipMemcpy(dst, data, n * (kind < 2 ? 8 : 4), hipMemcpyHostToDevice) != hipSuccess) { e = "uploading checkpoint " + path + " failed"; return MC_E_NO_DEVICE; }
      return 0;
    };
    if (int rc = ckpt::read_gen_body(in, g, (uint64_t)levels.front().states, kCkptChunkBytes, upload, err)) return rc;
    c[C_GEN] = (u64)g.generated; c[C_GIN] = (u64)g.generated_in_model;
    for (int k = 0; k < nact(); ++k) { c.act_generated(k) = (u64)act_generated[k]; c.act_distinct(k) = (u64)act_distinct[k]; }
    c.words_used() = g.words; c.n_states() = g.total; c.n_committed() = g.total;
    if (hipMemcpy(a.ctr, c.h.data(), c.bytes(), hipMemcpyHostToDevice) != hipSuccess) { err = "counter write failed"; return MC_E_NO_DEVICE; }
    return 0;
  }

  // the behaviour from an initial state to state sid (~0: none), appended to r.trace
  void trace_to(u64 sid, RunResult& r) {
    std::vector<u64> path;
    while (sid != ~0ull && path.size() < 100000) {
      path.push_back(sid);
      u64 p = ~0ull;
      (void)hipMemcpy(&p, d_parent_ + sid, 8, hipMemcpyDeviceToHost);
      sid = p;
    }
    for (size_t i = path.size(); i-- > 0;) trace_step(path[i], r);
  }
  void trace_step(u64 sid, RunResult& r) {
    u64 off = 0, par = 0;
    u32 act = 0;
    (void)hipMemcpy(&off, d_offs_ + sid, 8, hipMemcpyDeviceToHost);
    (void)hipMemcpy(&par, d_parent_ + sid, 8, hipMemcpyDeviceToHost);
    (void)hipMemcpy(&act, d_act_ + sid, 4, hipMemcpyDeviceToHost);
    std::vector<u32> w(std::min<u64>(1u << 20, words_stored - off));
    (void)hipMemcpy(w.data(), d_words_ + off, w.size() * 4, hipMemcpyDeviceToHost);
    r.trace.push_back({par == ~0ull ? "Initial predicate" : action_name(act), state_text(w.data(), "\n")});
  }

  int dump_states(const std::string& path, std::string& err) override {
    if (!d_words_) { err = "no run"; return MC_E_STATE; }
    if (!store_complete) { err = "the state store overflowed: the stored states are incomplete"; return MC_E_STATE; }
    std::vector<u32> w(words_stored);
    std::vector<u64> off(n_stored);
    HIPOK(hipMemcpy(w.data(), d_words_, w.size() * 4, hipMemcpyDeviceToHost));
    HIPOK(hipMemcpy(off.data(), d_offs_, off.size() * 8, hipMemcpyDeviceToHost));
    FILE* f = std::fopen(path.c_str(), "w");
    if (!f) { err = "cannot write " + path; return MC_E_IO; }
    for (u64 i = 0; i < n_stored; ++i) std::fprintf(f, "%s\n", state_text(w.data() + off[i], " ").c_str());
    std::fclose(f);
    return 0;
  }

  // single-GPU only: the sharded entry points are the hand-compiled families' (backend.h refuses the rest)
  int shard_open(const RunOpts&, int, int, std::string& err) override { err = "the generated path runs on one GPU"; return MC_E_UNSUPPORTED; }
  const RunResult* shard_result() const override { return &last; }
};

}  // namespace

Backend* make_tlagen_backend(const std::string& tla_path, const CfgFile& cfg) { return new TlagenBackend(tla_path, cfg); }

}  // namespace rmc
