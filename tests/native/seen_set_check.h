// TEST HARNESS ONLY (never part of the product).  Shared by orig_seen_set_check.hip and
// memb_seen_set_check.hip: the seeded generator, the case report (one JSON line per case), the
// perturbation bookkeeping of --host-only, and the checked HIP calls.
//
// A case is  inputs -> outputs -> check(inputs, outputs).  The outputs come from the product
// kernel (default) or from a sequential host routine that plays the kernel (--host-only, which
// makes no HIP call).  The check functions see only host vectors; their models are plain
// sequential containers (unordered_map fp -> minimum key, set, serial prefix sum).
#pragma once
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <set>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

namespace ssc {
using u64 = uint64_t;
using u32 = uint32_t;

struct Rng {   // splitmix64
  u64 s;
  explicit Rng(u64 seed) : s(seed) {}
  u64 next() {
    u64 z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  u64 below(u64 n) { return next() % n; }
  u64 fp() { u64 v; do v = next(); while (v == 0); return v; }   // 0 means "empty" everywhere
  template <class T>
  void shuffle(std::vector<T>& v) {
    for (size_t i = v.size(); i > 1; --i) std::swap(v[i - 1], v[below(i)]);
  }
};

inline std::string fmt(const char* f, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, f);
  std::vsnprintf(buf, sizeof buf, f, ap);
  va_end(ap);
  return buf;
}

// the perturbations of --host-only (tests/test_seen_set_cases.py holds the same list)
enum Perturb { P_DROP, P_DUP, P_KEY_RAISED, P_COUNT_TWICE, P_SWAP, P_WOFF, P_NPERTURB };
inline const char* perturb_name(int p) {
  static const char* n[] = {"record_dropped", "record_duplicated", "key_raised", "insertion_counted_twice",
                            "newrec_swapped", "woff_off_by_one"};
  return n[p];
}

struct Report {
  std::string name;
  u64 n = 0, distinct = 0;
  std::string first;                                   // first mismatch ("" = the contract holds)
  std::map<std::string, long long> props;              // what the case is named for (--host-only prints them)
  std::map<std::string, bool> rejected;                // perturbation -> the checker rejected it
  void fail(const std::string& m) { if (first.empty()) first = m; }
  void print() const {
    std::string esc;
    for (char c : first) { if (c == '"' || c == '\\') esc += '\\'; esc += c; }
    std::printf("{\"case\": \"%s\", \"ok\": %s, \"n\": %llu, \"distinct\": %llu, \"first_mismatch\": \"%s\", \"props\": {", name.c_str(),
                first.empty() ? "true" : "false", (unsigned long long)n, (unsigned long long)distinct, esc.c_str());
    bool c = false;
    for (auto& p : props) { std::printf("%s\"%s\": %lld", c ? ", " : "", p.first.c_str(), p.second); c = true; }
    std::printf("}, \"rejected\": {");
    c = false;
    for (auto& p : rejected) { std::printf("%s\"%s\": %s", c ? ", " : "", p.first.c_str(), p.second ? "true" : "false"); c = true; }
    std::printf("}}\n");
    std::fflush(stdout);
  }
};

// --host-only: out is the sequential routine's output, which passed check.  Apply one perturbation to a
// copy and record whether check rejects it.  mutate returns false where the case has nothing to perturb.
template <class Out, class Check>
void try_perturb(Report& r, int which, const Out& good, Check&& check, const std::function<bool(Out&)>& mutate) {
  Out bad = good;
  if (!mutate(bad)) return;
  r.rejected[perturb_name(which)] = !check(bad).empty();
}

// a fingerprint's LDS window (WIN slots from its home, SLOTS-slot set) can be full only if at least WIN other
// distinct fingerprints of its workgroup have their home within WIN - 1 slots of its own: the plain model
// of "the window was full" (no probing; a necessary condition, which is what the contracts need)
struct WindowModel {
  std::unordered_map<u32, u32> per_home;   // home -> distinct fingerprints
  u32 slots, win;
  WindowModel(const std::set<u64>& fps, u32 slots_, u32 win_) : slots(slots_), win(win_) {
    for (u64 f : fps) ++per_home[home(f)];
  }
  u32 home(u64 fp) const { return (u32)(fp >> 20) & (slots - 1); }
  bool may_be_full(u64 fp) const {
    u32 others = 0;
    const u32 h = home(fp);
    for (u32 d = 0; d < 2 * win - 1; ++d) {
      auto it = per_home.find((h + slots - (win - 1) + d) & (slots - 1));
      if (it != per_home.end()) others += it->second;
    }
    return others - 1 >= win;
  }
  u32 max_per_home() const { u32 m = 0; for (auto& p : per_home) m = p.second > m ? p.second : m; return m; }
};

// serial exclusive prefix sum; returns the total
template <class T, class O>
u64 serial_scan(const std::vector<T>& v, std::vector<O>& out) {
  u64 run = 0;
  out.resize(v.size());
  for (size_t i = 0; i < v.size(); ++i) { out[i] = (O)run; run += v[i]; }
  return run;
}

}  // namespace ssc

// Every HIP call of the check programs goes through this: on the first failure say what failed and exit
// non-zero, launching nothing more.
#define SSC_HIP(x)                                                                                    \
  do {                                                                                                \
    hipError_t e_ = (x);                                                                              \
    if (e_ != hipSuccess) {                                                                           \
      std::printf("{\"error\": \"%s: %s\"}\n", #x, hipGetErrorString(e_));                            \
      std::fflush(stdout);                                                                            \
      std::exit(2);                                                                                   \
    }                                                                                                 \
  } while (0)

#ifdef __HIPCC__
namespace ssc {
// device buffer filled from / read back into a host vector
template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  explicit DevBuf(const std::vector<T>& h) : n(h.size()) {
    SSC_HIP(hipMalloc(&p, (n ? n : 1) * sizeof(T)));
    if (n) SSC_HIP(hipMemcpy(p, h.data(), n * sizeof(T), hipMemcpyHostToDevice));
  }
  DevBuf(const DevBuf&) = delete;
  ~DevBuf() { (void)hipFree(p); }
  std::vector<T> get() const {
    std::vector<T> h(n);
    if (n) SSC_HIP(hipMemcpy(h.data(), p, n * sizeof(T), hipMemcpyDeviceToHost));
    return h;
  }
};
inline void launched(const char* what) {
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    std::printf("{\"error\": \"%s: %s\"}\n", what, hipGetErrorString(e));
    std::fflush(stdout);
    std::exit(2);
  }
}
}  // namespace ssc
#endif
