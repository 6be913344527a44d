// raftmc host: the state store every spec backend owns.  Stored states and
// their parent pointers by global id: [0, base) in host memory (the completed levels a spill or a
// recovered checkpoint put there, host_store.h), [base, total) in two device arrays of cap slots.
// Off the per-level hot path: the level loops take the raw device pointers and index them themselves.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <utility>

#include "ckpt_file.h"
#include "common.h"
#include "host_store.h"

namespace rmc {

class StateStore {
 public:
  static constexpr u64 kBlock = 1u << 20;   // states per device<->host block
  StateStore() {}
  StateStore(const StateStore&) = delete;
  StateStore& operator=(const StateStore&) = delete;
  ~StateStore() { release(); }

  hipError_t alloc(u64 cap, int words) {
    release();
    words_ = (u64)words; host_.set_words(words); cap_ = cap;
    const hipError_t e = hipMalloc(&d_states_, cap * words_ * 4);
    return e == hipSuccess ? hipMalloc(&d_meta_, cap * 8) : e;
  }
  void release() {
    (void)hipFree(d_states_); (void)hipFree(d_meta_);   // (a null pointer is a no-op)
    d_states_ = nullptr; d_meta_ = nullptr; cap_ = 0; total_ = 0;
    reset();
  }
  // every stored state on the device again, none on the host
  void reset() { base_ = 0; host_.clear(); }

  u32* states() const { return d_states_; }   // device slot 0 holds global id base()
  u64* meta() const { return d_meta_; }
  u64 base() const { return base_; }
  u64 cap() const { return cap_; }
  u64 total() const { return total_; }   // stored states, both parts
  void set_total(u64 n) { total_ = n; }

  // stored state `gid` and its parent pointer, from the host part or the device
  bool read(u64 gid, u32* words, u64* meta) const {
    const u64 d = gid - base_;
    if (gid >= base_) return hipMemcpy(words, d_states_ + d * words_, words_ * 4, hipMemcpyDeviceToHost) == hipSuccess &&
                             hipMemcpy(meta, d_meta_ + d, 8, hipMemcpyDeviceToHost) == hipSuccess;
    std::memcpy(words, host_.state(gid), words_ * 4);
    *meta = host_.meta(gid);
    return true;
  }

  // move the completed levels [base, level_begin) to host memory and the frontier to the front of
  // the device store (left shift by d in blocks of <= d slots: each block's target only overlaps
  // blocks already moved)
  int spill(u64 level_begin, u64 level_count, hipStream_t stream, bool progress, std::string& err) {
    const u64 d = level_begin - base_;
    u32* hs = nullptr; u64* hm = nullptr;
    const auto ts = std::chrono::steady_clock::now();
    auto since = [&]() { return std::chrono::duration<double>(std::chrono::steady_clock::now() - ts).count(); };
    host_.append(d, &hs, &hm);   // a segment of its own: the host part is never reallocated
    if (progress) std::fprintf(stderr, "spill: %.1f GB of host memory allocated in %.3f s\n", d * (words_ * 4.0 + 8) / 1e9, since());
    bool ok = hipStreamSynchronize(stream) == hipSuccess && hipMemcpy(hs, d_states_, d * words_ * 4, hipMemcpyDeviceToHost) == hipSuccess &&
              hipMemcpy(hm, d_meta_, d * 8, hipMemcpyDeviceToHost) == hipSuccess;
    if (ok && progress) std::fprintf(stderr, "spill: copied to host at %.3f s\n", since());
    for (u64 off = 0; ok && off < level_count; off += d) {
      const u64 n = std::min<u64>(d, level_count - off);
      ok = hipMemcpyAsync(d_states_ + off * words_, d_states_ + (d + off) * words_, n * words_ * 4, hipMemcpyDeviceToDevice, stream) == hipSuccess &&
           hipMemcpyAsync(d_meta_ + off, d_meta_ + d + off, n * 8, hipMemcpyDeviceToDevice, stream) == hipSuccess &&
           hipStreamSynchronize(stream) == hipSuccess;
    }
    if (!ok) { err = std::string("state store spill: ") + hipGetErrorString(hipGetLastError()); return MC_E_NO_DEVICE; }
    base_ = level_begin;
    return 0;
  }

  // fn(gid, words) over [0, total) in global-id order: the host segments, then the device part
  // block by block (no second copy of the store in host memory); false when a device copy failed
  template <int NWP, class F>
  bool for_each_state(F fn) const {
    auto each = [&](u64 g0, u64 n, const u32* st) {
      for (u64 k = 0; k < n; ++k) fn(g0 + k, *reinterpret_cast<const u32(*)[NWP]>(st + k * NWP));
      return true;
    };
    host_.for_each_segment([&](u64 g0, u64 n, const u32* st, const u64*) { each(g0, n, st); });
    return blocks(true, d_states_, NWP, total_ - base_, [&](const u32* buf, u64 first, u64 n) { return each(base_ + first, n, buf); });
  }

  // the checkpoint body (ckpt_file.h): the states [0, total), then their parent pointers
  bool write_body(FILE* f) const {
    return host_.write_states(f) && blocks(true, d_states_, words_, total_ - base_, FileIo{f, true, words_}) &&
           host_.write_meta(f) && blocks(true, (u32*)d_meta_, 2, total_ - base_, FileIo{f, true, 2});
  }
  // ... read back: the completed levels [0, level_begin) into one host segment when the device
  // store cannot hold all `total` states (as after a spill), the rest into the device store.  The
  // seen-set is the backend's: reinsert(device states, n) queues its kernel on `stream`, for the
  // host part staged through the backend's idle device buffer `stage` (stage_states states at a
  // time), then once for the device part; the kernels flag a full table in the device word
  // `table_full`.  On any failure the store is left reset().
  template <class R>
  int read_body(const ckpt::Reader& in, u64 total, u64 level_begin, void* stage, u64 stage_states, hipStream_t stream,
                const u64* table_full, R reinsert, std::string& err) {
    reset();
    const u64 lb = total > cap_ ? level_begin : 0;
    if (level_begin > total || total - lb > cap_) { err = "checkpoint frontier exceeds the state store (raise state_store_bytes)"; return MC_E_OOM; }
    FILE* f = in.file();
    u32* hs = nullptr; u64* hm = nullptr;
    if (lb) host_.append(lb, &hs, &hm);
    const FileIo st{f, false, words_}, me{f, false, 2};
    const bool ok = st(hs, 0, lb) && blocks(false, d_states_, words_, total - lb, st) &&
                    me((u32*)hm, 0, lb) && blocks(false, (u32*)d_meta_, 2, total - lb, me);
    if (!ok) { reset(); return in.truncated(err); }
    bool dev = true;
    for (u64 b = 0; dev && b < lb; b += stage_states) {
      const u64 n = std::min<u64>(stage_states, lb - b);
      dev = hipMemcpy(stage, hs + b * words_, n * words_ * 4, hipMemcpyHostToDevice) == hipSuccess;
      if (dev) reinsert((const u32*)stage, n);
      dev = dev && hipGetLastError() == hipSuccess && hipStreamSynchronize(stream) == hipSuccess;
    }
    if (dev && total > lb) reinsert((const u32*)d_states_, total - lb);
    u64 full = 0;
    dev = dev && hipGetLastError() == hipSuccess && hipMemcpyAsync(&full, table_full, 8, hipMemcpyDeviceToHost, stream) == hipSuccess &&
          hipStreamSynchronize(stream) == hipSuccess;
    if (!dev || full) {
      reset();
      err = dev ? "fingerprint table too small for the checkpoint (raise fp_table_bytes)" : "checkpoint seen-set rebuild failed";
      return dev ? MC_E_OOM : MC_E_NO_DEVICE;
    }
    base_ = lb; total_ = total;
    return 0;
  }

 private:
  struct FileIo {   // io for blocks(): n states of `words` words each to (write) or from the file
    FILE* f; bool write; u64 words;
    bool operator()(u32* buf, u64, u64 n) const { return (write ? std::fwrite(buf, 4, n * words, f) : std::fread(buf, 4, n * words, f)) == n * words; }
  };
  // n states of one device array (words 32-bit words per state) through one bounce buffer, kBlock
  // states at a time: io(buffer, first state, count) runs behind the copy to the host (to_host) or
  // fills the buffer ahead of the copy to the device; false when io or a copy failed
  template <class F>
  static bool blocks(bool to_host, u32* dev, u64 words, u64 n, F io) {
    std::vector<u32> buf(std::min(n, kBlock) * words);
    for (u64 b = 0; b < n; b += kBlock) {
      const u64 m = std::min(kBlock, n - b);
      u32* const d = dev + b * words;
      const bool ok = to_host ? hipMemcpy(buf.data(), d, m * words * 4, hipMemcpyDeviceToHost) == hipSuccess && io(buf.data(), b, m)
                              : io(buf.data(), b, m) && hipMemcpy(d, buf.data(), m * words * 4, hipMemcpyHostToDevice) == hipSuccess;
      if (!ok) return false;
    }
    return true;
  }

  u32* d_states_ = nullptr; u64* d_meta_ = nullptr;
  u64 words_ = 0, cap_ = 0, total_ = 0;
  // completed levels moved to host memory: global ids [0, base_) live in host_ (segments)
  u64 base_ = 0;
  HostStore host_;
};

// Parent-pointer chase on the host (<= depth reads of one state each): the trace that ends in stored
// state `parent` (and, when last_act names its action, the event's successor `last_text`), oldest
// first.  A parent pointer holds the action (act_names) at act_shift / act_mask and the parent's
// global id from gid_shift up; ~0 marks the initial state.  A failed readback says so in err.
template <int NWP, class Text>
void build_trace(const StateStore& store, u64 parent, const char* last_act, const std::string& last_text, Text text,
                 const char* const* act_names, int act_shift, u64 act_mask, int gid_shift,
                 std::vector<std::pair<std::string, std::string>>& trace, std::string& err) {
  trace.clear();
  if (last_act) trace.push_back({last_act, last_text});
  u64 g = parent;
  while (true) {
    u32 w[NWP]; u64 meta = 0;
    if (!store.read(g, w, &meta)) { err = "trace readback failed"; break; }
    if (meta == ~0ull) { trace.push_back({"<Initial predicate>", text(w)}); break; }
    trace.push_back({act_names[(meta >> act_shift) & act_mask], text(w)});
    g = meta >> gid_shift;
  }
  std::reverse(trace.begin(), trace.end());
}

// mc_dump_states: one line of text(words) per stored state, in global-id order
template <int NWP, class Text>
int dump_states(const StateStore& store, const std::string& path, Text text, std::string& err) {
  const ckpt::File f = ckpt::open_file(path, "w");
  if (!f) { err = "cannot write " + path; return MC_E_IO; }
  if (store.for_each_state<NWP>([&](u64, const u32 (&w)[NWP]) { std::fprintf(f.get(), "%s\n", text(w).c_str()); })) return 0;
  err = "mc_dump_states: state readback failed";
  return MC_E_NO_DEVICE;
}

}  // namespace rmc
