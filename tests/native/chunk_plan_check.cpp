// The level plan of the single-GPU -workers N search (csrc/chunk_plan.h) on the host: which parents
// each (sub-)chunk takes and which half of the record buffers it uses.  Built with
// -fsanitize=address,undefined and run directly (tests/test_chunk_plan.py).
//   chunk_plan_check        prints "ok" and exits 0, or says what failed
#include <cstdio>

#include "chunk_plan.h"

using namespace rmc;

static int fails = 0;
#define CHECK(x) \
  do { if (!(x)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed (full %llu, sub %llu, threshold %llu, level %llu)\n", __FILE__, __LINE__, #x, \
                                (unsigned long long)g_full, (unsigned long long)g_sub, (unsigned long long)g_thr, (unsigned long long)g_level); ++fails; } } while (0)

static uint64_t g_full, g_sub, g_thr, g_level;
static constexpr uint64_t WG = 256;

// today's chunking: whole-allocation chunks from buffer 0
static void check_unsplit(const std::vector<Chunk>& c, uint64_t level, uint64_t full) {
  CHECK(c.size() == (level + full - 1) / full);
  for (size_t i = 0; i < c.size(); ++i) {
    CHECK(c[i].buffer == 0);
    CHECK(c[i].first == i * full);
    CHECK(c[i].count == (i + 1 < c.size() ? full : level - i * full));
  }
}

static void check(uint64_t full, uint64_t sub, uint64_t thr, uint64_t level) {
  g_full = full; g_sub = sub; g_thr = thr; g_level = level;
  const ChunkPlan p(full, sub, thr, (int)WG);
  CHECK(p.full_cap == full && p.half_cap % WG == 0 && 2 * p.half_cap <= full && p.half_cap + WG > full / 2);
  std::vector<Chunk> c(3, Chunk{7, 7, 7});   // plan() replaces what the vector held
  const bool split = p.plan(level, c);
  CHECK(!c.empty());
  // the chunks cover the level exactly, in order
  uint64_t next = 0;
  for (const Chunk& k : c) { CHECK(k.first == next); CHECK(k.count > 0); next += k.count; }
  CHECK(next == level);
  // every count but the last is a whole number of workgroups
  for (size_t i = 0; i + 1 < c.size(); ++i) CHECK(c[i].count % WG == 0);
  if (sub == 0) { CHECK(!split); check_unsplit(c, level, full); return; }
  const uint64_t sub_eff = (sub + WG - 1) / WG * WG < p.half_cap ? (sub + WG - 1) / WG * WG : p.half_cap;
  CHECK(p.sub == sub_eff && p.sub >= WG);
  if (level < thr || level <= sub_eff) {   // under the threshold, or one sub-chunk: as today
    CHECK(!split);
    check_unsplit(c, level, full);
    if (level <= full) CHECK(c.size() == 1);
    return;
  }
  CHECK(split && c.size() >= 2);
  for (size_t i = 0; i < c.size(); ++i) {
    CHECK(c[i].count <= p.half_cap);          // none exceeds the half buffer
    CHECK(c[i].buffer == (int)(i & 1));       // buffers alternate
    if (i + 1 < c.size()) CHECK(c[i].count == sub_eff);
  }
}

int main() {
  // smallest allocation, an odd number of workgroups, C2's under the library's default store, orig_scan's limit
  const uint64_t fulls[] = {4096, 4096 + 256, 4953600, 16777216};
  const uint64_t subs[] = {0, 1, 256, 768, OVERLAP_STATES, ~0ull >> 1};
  for (uint64_t full : fulls) {
    const uint64_t half = full / 2 / WG * WG;
    const uint64_t thrs[] = {0, 300, OVERLAP_MIN_LEVEL};
    for (uint64_t sub : subs)
      for (uint64_t thr : thrs) {
        const uint64_t levels[] = {1, 255, 256, 257, 767, 768, 769, thr ? thr - 1 : 1, thr ? thr : 1, thr + 1, 10072911,
                                   half, half + 1, 7 * half + 1, full - 1, full, full + 1, 3 * full + 1,
                                   OVERLAP_STATES - 1, OVERLAP_STATES, OVERLAP_STATES + 1, 2 * OVERLAP_STATES + 1};
        for (uint64_t level : levels) check(full, sub, thr, level);
      }
  }
  // the forced sizes of tests/test_gpu_overlap.py on the smallest allocation: a level of 8 710 parents
  // at 256 is 35 sub-chunks, the last of 6 parents in buffer 0
  {
    const ChunkPlan p(4096, 256, 0);
    std::vector<Chunk> c;
    g_full = 4096; g_sub = 256; g_thr = 0; g_level = 8710;
    CHECK(p.plan(8710, c) && c.size() == 35 && c.back().first == 8704 && c.back().count == 6 && c.back().buffer == 0);
    CHECK(!p.plan(256, c) && c.size() == 1);
    CHECK(p.plan(257, c) && c.size() == 2 && c[1].count == 1 && c[1].buffer == 1);
  }
  // the default size: the half buffer, and only where a half holds OVERLAP_MIN_HALF parents
  {
    g_sub = OVERLAP_STATES; g_thr = OVERLAP_MIN_LEVEL; g_level = 0;
    g_full = 4096;            CHECK(ChunkPlan::default_sub(g_full) == 0);
    g_full = (4u << 20) - 256; CHECK(ChunkPlan::default_sub(g_full) == 0);
    g_full = 4u << 20;        CHECK(ChunkPlan::default_sub(g_full) == OVERLAP_STATES);
    g_full = 4953600;         CHECK(ChunkPlan::default_sub(g_full) == OVERLAP_STATES);
    const ChunkPlan p(4953600, ChunkPlan::default_sub(4953600), OVERLAP_MIN_LEVEL);
    std::vector<Chunk> c;
    CHECK(p.sub == p.half_cap && p.half_cap == 2476800);
    g_level = 3719733;  CHECK(!p.plan(g_level, c) && c.size() == 1);                 // under the threshold
    g_level = 10072911; CHECK(p.plan(g_level, c) && c.size() == 5 && c[4].count == 10072911 - 4 * 2476800ull && c[4].buffer == 0);
  }
  if (fails) return 1;
  std::puts("ok");
  return 0;
}
