// The index arithmetic of a recovery at another GPU count (csrc/reshard_plan.h) on the host, as the
// kernels of csrc/orig_reshard.hip use it: canonical order, old id -> position in its level, stable
// index per new owner, new ids, rewritten parent pointers.  tests/test_reshard_plan.py writes a
// source, runs this and compares with its own brute-force restatement.
//   reshard_plan_check IN
// IN (whitespace-separated unsigned numbers): W W' L, then per level: W slice sizes, then per state
// of the level in the canonical order its new owner and its parent pointer (source ids).
// Prints per level "level <owner counts...>" and per state "<new id> <new parent pointer>", or
// "<new id> bad" for a parent pointer that names no state of the level before.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "reshard_plan.h"

using namespace rmc;

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: reshard_plan_check IN\n"); return 2; }
  FILE* f = std::fopen(argv[1], "r");
  if (!f) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  auto next = [&]() { unsigned long long v = 0; if (std::fscanf(f, "%llu", &v) != 1) { std::fprintf(stderr, "short input\n"); std::exit(2); } return (u64)v; };
  const u64 W = next(), WP = next(), L = next();
  if (W < 1 || W > (u64)RESHARD_MAX_WORLD || WP < 1 || WP > (u64)RESHARD_MAX_WORLD) { std::fprintf(stderr, "bad world\n"); return 2; }
  ReshardLevel prev = {}, cur = {};
  std::vector<u64> map_prev, map_cur;
  u64 owner_begin[RESHARD_MAX_WORLD] = {0};
  for (u64 l = 0; l < L; ++l) {
    cur.world = (u32)W;
    for (u64 r = 0; r < W; ++r) { cur.begin[r] += l ? prev.count[r] : 0; cur.count[r] = next(); }
    const u64 n = reshard_canonical(cur);
    map_cur.assign(n, 0);
    u64 run[RESHARD_MAX_WORLD] = {0};
    std::vector<u64> metas(n);
    for (u64 i = 0; i < n; ++i) {
      const u64 owner = next();
      metas[i] = next();
      if (owner >= WP) { std::fprintf(stderr, "bad owner\n"); return 2; }
      map_cur[i] = reshard_new_id((u32)owner, owner_begin[owner], run[owner]++);
    }
    std::printf("level");
    for (u64 o = 0; o < WP; ++o) std::printf(" %" PRIu64, run[o]);
    std::printf("\n");
    for (u64 i = 0; i < n; ++i) {
      u64 pos = 0;
      if (metas[i] == ~0ull) std::printf("%" PRIu64 " %" PRIu64 "\n", map_cur[i], metas[i]);
      else if (reshard_position(prev, metas[i] >> META_GID_SHIFT, pos) && pos < map_prev.size())
        std::printf("%" PRIu64 " %" PRIu64 "\n", map_cur[i], reshard_meta(metas[i], map_prev[pos]));
      else std::printf("%" PRIu64 " bad\n", map_cur[i]);
    }
    for (u64 o = 0; o < WP; ++o) owner_begin[o] += run[o];
    prev = cur;
    map_prev.swap(map_cur);
  }
  std::fclose(f);
  return 0;
}
