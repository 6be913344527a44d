// The owner of a backend's device resources (csrc/dev_owner.h) on the host, over a counting
// stand-in for the runtime that can refuse the k-th creation.  Built with
// -fsanitize=address,undefined and run directly (tests/test_dev_owner.py).
//   dev_owner_check        prints "ok" and exits 0, or says what failed
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "dev_owner.h"

using namespace rmc;

static int fails = 0;
#define CHECK(x) \
  do { if (!(x)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); ++fails; } } while (0)

// every handle is a heap block of its own: a double free or a leak is also the sanitizer's finding
struct CountingApi {
  using error = int;
  static constexpr error ok = 0;
  static std::set<void*> live[4];
  static std::vector<DevRes> order;                 // the kinds, as they were destroyed
  static int created, destroyed, wrong, fail_at;   // fail_at: the creation (from 0) that is refused, -1 none
  static error create(DevRes kind, void** h, size_t) {
    if (created == fail_at) { fail_at = -1; *h = (void*)0x1;   /* garbage the owner must not keep */ return 2; }
    *h = std::malloc(8);
    live[(int)kind].insert(*h);
    ++created;
    return ok;
  }
  static void destroy(DevRes kind, void* h) {
    if (!live[(int)kind].erase(h)) { ++wrong; return; }   // never created, destroyed twice, or as another kind
    std::free(h);
    order.push_back(kind);
    ++destroyed;
  }
  static size_t alive() { return live[0].size() + live[1].size() + live[2].size() + live[3].size(); }
  static void reset() { created = destroyed = wrong = 0; fail_at = -1; order.clear(); }
};
std::set<void*> CountingApi::live[4];
std::vector<DevRes> CountingApi::order;
int CountingApi::created, CountingApi::destroyed, CountingApi::wrong, CountingApi::fail_at = -1;

using Owner = DevOwner<CountingApi>;

// a backend's handles, allocated in ensure_alloc's style: the first failure returns
struct Handles {
  char* a = nullptr; long* b = nullptr; int* pinned = nullptr;
  struct Ev* ev = nullptr; struct St* st0 = nullptr; struct St* st1 = nullptr;
  static constexpr int N = 6;
  int alloc(Owner& o) {
    if (o.device(&a, 16)) return 1;
    if (o.stream(&st0, 1)) return 1;   // a stream in the middle: release() still destroys it last
    if (o.device(&b, 32)) return 1;
    if (o.pinned(&pinned, 8)) return 1;
    if (o.event(&ev)) return 1;
    if (o.stream(&st1, 1)) return 1;
    return 0;
  }
  bool all_null() const { return !a && !b && !pinned && !ev && !st0 && !st1; }
};

int main() {
  // a failure after k of n creations releases exactly k, once; release() twice is clean
  for (int k = 0; k <= Handles::N; ++k) {
    CountingApi::reset();
    CountingApi::fail_at = k < Handles::N ? k : -1;
    Handles h;
    {
      Owner o;
      CHECK(h.alloc(o) == (k < Handles::N ? 1 : 0));
      CHECK(CountingApi::created == k && (int)CountingApi::alive() == k && (int)o.size() == k);
      o.release();
      CHECK(CountingApi::destroyed == k && CountingApi::alive() == 0 && CountingApi::wrong == 0);
      CHECK(h.all_null() && o.size() == 0);
      o.release();
      CHECK(CountingApi::destroyed == k && CountingApi::wrong == 0);
      // the next allocation after a failed one starts clean
      CHECK(h.alloc(o) == 0 && (int)CountingApi::alive() == Handles::N);
    }   // the destructor releases
    CHECK(CountingApi::alive() == 0 && CountingApi::wrong == 0 && h.all_null());
    CHECK(CountingApi::created == CountingApi::destroyed);
  }
  // streams go last, whatever the creation order; the pool's events go with the rest
  {
    CountingApi::reset();
    Handles h;
    Owner o;
    CHECK(h.alloc(o) == 0);
    CHECK(o.pool_event(3) != nullptr && o.pool_event(3) == o.pool_event(3));   // four pool events, made once
    CHECK(CountingApi::live[(int)DevRes::Event].size() == 5);
    o.release();
    CHECK(CountingApi::order.size() == Handles::N + 4);
    for (size_t i = 0; i < CountingApi::order.size(); ++i)
      CHECK((CountingApi::order[i] == DevRes::Stream) == (i >= CountingApi::order.size() - 2));
    CHECK(CountingApi::alive() == 0 && CountingApi::wrong == 0 && h.all_null());
  }
  // a handle is freed and re-created in place, registered once
  {
    CountingApi::reset();
    Handles h;
    Owner o;
    CHECK(h.alloc(o) == 0);
    const size_t n = o.size();
    o.free(&h.b);
    CHECK(!h.b && CountingApi::destroyed == 1);
    o.free(&h.b);   // again: a no-op
    CHECK(CountingApi::destroyed == 1 && CountingApi::wrong == 0);
    CHECK(o.device(&h.b, 64) == 0 && h.b && o.size() == n);
    CHECK(o.device(&h.b, 128) == 0 && h.b && o.size() == n);   // over a set handle: the old block is freed first
    CHECK(CountingApi::destroyed == 2 && (int)CountingApi::alive() == Handles::N);
    CountingApi::fail_at = CountingApi::created;               // a refused re-creation leaves the handle null
    CHECK(o.device(&h.b, 256) != 0 && !h.b && (int)CountingApi::alive() == Handles::N - 1);
    o.release();
    CHECK(CountingApi::alive() == 0 && CountingApi::wrong == 0 && h.all_null());
  }
  // moved-from is empty; the target owns everything, and an assigned-over owner releases its own first
  {
    CountingApi::reset();
    Handles h, h2;
    Owner o;
    CHECK(h.alloc(o) == 0);
    (void)o.pool_event(1);
    Owner p(std::move(o));
    CHECK(o.size() == 0 && (int)p.size() == Handles::N + 2);
    o.release();   // nothing to release
    CHECK((int)CountingApi::alive() == Handles::N + 2 && CountingApi::destroyed == 0);
    Owner q;
    CHECK(h2.alloc(q) == 0);
    q = std::move(p);
    CHECK(p.size() == 0 && h2.all_null() && (int)CountingApi::alive() == Handles::N + 2);
    q.release();
    CHECK(CountingApi::alive() == 0 && CountingApi::wrong == 0 && h.all_null());
    CHECK(CountingApi::created == CountingApi::destroyed);
  }
  if (fails) return 1;
  std::puts("ok");
  return 0;
}
