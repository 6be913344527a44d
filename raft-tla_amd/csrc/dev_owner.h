// raftmc host: one owner for a backend's device resources.  The backend keeps its typed raw
// pointers and handles (the launch code indexes them); it creates each through this registry,
// which remembers where the handle lives, and release() walks the list: every resource is freed
// once and its handle nulled, with no hand-kept free list or nulling list.  A creation that
// fails leaves a null handle, so whatever was created before it is released as usual.
//
// Api: the runtime, as static members (HipDevApi below; the stand-alone check of this header,
// tests/native/dev_owner_check.cpp, counts calls instead):
//   using error = ...;  static constexpr error ok = ...;
//   static error create(DevRes kind, void** handle, size_t arg);   // arg: bytes, or creation flags
//   static void destroy(DevRes kind, void* handle);
#pragma once
#include <cstddef>
#include <utility>
#include <vector>

namespace rmc {

enum class DevRes { Device, Pinned, Event, Stream };

template <class Api>
class DevOwner {
 public:
  using error = typename Api::error;
  DevOwner() = default;
  DevOwner(const DevOwner&) = delete;
  DevOwner& operator=(const DevOwner&) = delete;
  DevOwner(DevOwner&& o) noexcept { take(o); }
  DevOwner& operator=(DevOwner&& o) noexcept {
    if (this != &o) { release(); take(o); }
    return *this;
  }
  ~DevOwner() { release(); }

  // *p (a member of the backend, alive as long as this owner) is freed first when it is set
  template <class T> error device(T** p, size_t bytes) { return create(DevRes::Device, (void**)p, bytes); }
  template <class T> error pinned(T** p, size_t bytes) { return create(DevRes::Pinned, (void**)p, bytes); }
  template <class H> error event(H** p, unsigned flags = 0) { return create(DevRes::Event, (void**)p, flags); }
  template <class H> error stream(H** p, unsigned flags) { return create(DevRes::Stream, (void**)p, flags); }

  // frees *p now and nulls it (no-op when null or not created here)
  template <class T> void free(T** p) {
    for (Slot& s : slots_)
      if (s.p == (void**)p) drop(s);
  }

  // event i of a pool that grows on demand (timing pairs); null when the runtime refuses one
  void* pool_event(size_t i) {
    while (pool_.size() <= i) {
      void* e = nullptr;
      if (Api::create(DevRes::Event, &e, 0) != Api::ok || !e) return nullptr;
      pool_.push_back(e);
    }
    return pool_[i];
  }

  // everything, newest first, streams after all else (the caller has synchronised them)
  void release() {
    for (int streams = 0; streams < 2; ++streams) {
      for (size_t i = slots_.size(); i-- > 0;)
        if ((slots_[i].kind == DevRes::Stream) == (streams == 1)) drop(slots_[i]);
      if (!streams) {
        for (size_t i = pool_.size(); i-- > 0;) Api::destroy(DevRes::Event, pool_[i]);
        pool_.clear();
      }
    }
    slots_.clear();
  }

  size_t size() const { return slots_.size() + pool_.size(); }

 private:
  struct Slot { void** p; DevRes kind; };
  std::vector<Slot> slots_;
  std::vector<void*> pool_;

  static void drop(Slot& s) {
    if (*s.p) Api::destroy(s.kind, *s.p);
    *s.p = nullptr;
  }
  void take(DevOwner& o) {
    slots_ = std::move(o.slots_); pool_ = std::move(o.pool_);
    o.slots_.clear(); o.pool_.clear();
  }
  error create(DevRes kind, void** p, size_t arg) {
    Slot* s = nullptr;
    for (Slot& q : slots_)
      if (q.p == p) s = &q;
    if (s) drop(*s);
    else *p = nullptr;
    const error e = Api::create(kind, p, arg);
    if (e != Api::ok) { *p = nullptr; return e; }
    if (!s) slots_.push_back({p, kind});
    return e;
  }
};

#ifdef HIP_INCLUDE_HIP_HIP_RUNTIME_H
struct HipDevApi {
  using error = hipError_t;
  static constexpr error ok = hipSuccess;
  static error create(DevRes kind, void** h, size_t arg) {
    switch (kind) {
      case DevRes::Device: return hipMalloc(h, arg);
      case DevRes::Pinned: return hipHostMalloc(h, arg, hipHostMallocDefault);
      case DevRes::Event: return hipEventCreateWithFlags((hipEvent_t*)h, (unsigned)arg);
      default: return hipStreamCreateWithFlags((hipStream_t*)h, (unsigned)arg);
    }
  }
  static void destroy(DevRes kind, void* h) {
    switch (kind) {
      case DevRes::Device: (void)hipFree(h); break;
      case DevRes::Pinned: (void)hipHostFree(h); break;
      case DevRes::Event: (void)hipEventDestroy((hipEvent_t)h); break;
      default: (void)hipStreamDestroy((hipStream_t)h); break;
    }
  }
};
#endif

}  // namespace rmc
