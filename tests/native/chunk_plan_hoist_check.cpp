// The level plan behind a level hoist (csrc/chunk_plan.h) on the host: a level whose
// first parents were generated ahead into one half of the record buffers.  Built with
// -fsanitize=address,undefined and run directly (tests/test_chunk_plan_hoist.py).
//   chunk_plan_hoist_check        prints "ok" and exits 0, or says what failed
#include <cstdio>

#include "chunk_plan.h"

using namespace rmc;

static int fails = 0;
static uint64_t g_full, g_sub, g_level, g_pre;
static int g_buf;
#define CHECK(x) \
  do { if (!(x)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed (full %llu, sub %llu, level %llu, prefix %llu in buffer %d)\n", __FILE__, __LINE__, #x, \
                                (unsigned long long)g_full, (unsigned long long)g_sub, (unsigned long long)g_level, (unsigned long long)g_pre, g_buf); ++fails; } } while (0)

static constexpr uint64_t WG = 256;

static void check(const ChunkPlan& p, uint64_t level, uint64_t pre, int buf) {
  g_level = level; g_pre = pre; g_buf = buf;
  std::vector<Chunk> c(3, Chunk{7, 7, 7});   // plan() replaces what the vector held
  const bool split = p.plan(level, c, pre, buf);
  if (pre == 0) {   // no prefix: today's plan, element for element
    std::vector<Chunk> t;
    CHECK(p.plan(level, t) == split && t.size() == c.size());
    for (size_t i = 0; i < c.size() && i < t.size(); ++i) CHECK(c[i].first == t[i].first && c[i].count == t[i].count && c[i].buffer == t[i].buffer);
    return;
  }
  // a prefix the level cannot have had (longer than the level, or a partial workgroup that is not the
  // level's end) gives no plan at all
  const bool ok = pre <= level && pre <= p.half_cap && (pre % WG == 0 || pre == level);
  CHECK(p.prefix_ok(level, pre) == ok);
  if (!ok) { CHECK(!split && c.empty()); return; }
  CHECK(split && !c.empty());
  // chunk 0 is the prefix, in its buffer
  CHECK(c[0].first == 0 && c[0].count == pre && c[0].buffer == buf);
  // the chunks cover [0, level) once, in order
  uint64_t next = 0;
  for (const Chunk& k : c) { CHECK(k.first == next); CHECK(k.count > 0); next += k.count; }
  CHECK(next == level);
  for (size_t i = 0; i < c.size(); ++i) {
    CHECK(c[i].buffer == 0 || c[i].buffer == 1);
    if (i) CHECK(c[i].buffer != c[i - 1].buffer);                       // neighbours alternate
    if (i + 1 < c.size()) CHECK(c[i].count % WG == 0);                  // whole workgroups but the last
    CHECK(c[i].count <= p.half_cap);
    if (i && i + 1 < c.size()) CHECK(c[i].count == p.sub);              // the rest as today: sub-chunks
  }
  CHECK(c.size() == 1 + (level - pre + p.sub - 1) / p.sub);
}

int main() {
  // the forced sizes of tests/test_gpu_level_hoist.py on the smallest allocation, and C2's under the
  // library's default store
  struct { uint64_t full, sub, thr; } const plans[] = {{4096, 256, 0}, {4096, 768, 0}, {4096 + 256, 768, 300},
                                                      {4953600, ChunkPlan::default_sub(4953600), OVERLAP_MIN_LEVEL}};
  for (const auto& pl : plans) {
    const ChunkPlan p(pl.full, pl.sub, pl.thr, (int)WG);
    g_full = pl.full; g_sub = p.sub;
    const uint64_t sub = p.sub;
    const uint64_t levels[] = {1, 255, 256, 257, sub - 1, sub, sub + 1, 2 * sub, 2 * sub + 1, 5 * sub + 17};
    const uint64_t pres[] = {0, 256, sub, p.half_cap};
    for (uint64_t level : levels)
      for (uint64_t pre : pres)
        for (int buf = 0; buf < 2; ++buf) check(p, level, pre, buf);
  }
  // C2's level 15 behind a hoist of one half into buffer 1: the prefix, then sub-chunks from buffer 0
  {
    const ChunkPlan p(4953600, ChunkPlan::default_sub(4953600), OVERLAP_MIN_LEVEL);
    std::vector<Chunk> c;
    g_full = 4953600; g_sub = p.sub; g_level = 10072911; g_pre = 2476800; g_buf = 1;
    CHECK(p.plan(g_level, c, g_pre, g_buf) && c.size() == 5 && c[0].buffer == 1 && c[1].first == 2476800 && c[1].buffer == 0 &&
          c[4].count == 10072911 - 4 * 2476800ull && c[4].buffer == 1);
    g_pre = 1000192;   // a shorter one: 3907 workgroups
    CHECK(p.plan(g_level, c, g_pre, 0) && c.size() == 5 && c[1].first == 1000192 && c[1].count == 2476800 && c[1].buffer == 1 &&
          c[4].first == 1000192 + 3 * 2476800ull && c[4].count == 10072911 - 1000192 - 3 * 2476800ull);
    // a plan that never splits has no halves to hoist into
    const ChunkPlan one(4096, 0, 0);
    g_full = 4096; g_sub = 0; g_level = 4096; g_pre = 256;
    CHECK(!one.prefix_ok(4096, 256) && !one.plan(4096, c, 256, 0) && c.empty());
  }
  if (fails) return 1;
  std::puts("ok");
  return 0;
}
