// The multi-GPU checkpoint files (csrc/ckpt_file.h: manifest, rank files, ckpt::open_source) on the
// host: a round trip, the manifest cut at every length, a rank file cut short, a wrong world,
// generation or rank, a missing rank file, level tables that disagree, and a single-GPU file as a
// one-part source.  Built with -fsanitize=address,undefined and run directly
// (tests/test_shard_ckpt_file.py).
//   shard_ckpt_check DIR     (an empty scratch directory)      prints "ok" and exits 0, or says what failed
#include <sys/stat.h>
#include <unistd.h>

#include <cstdlib>

#include "ckpt_file.h"

using namespace rmc;

static int fails = 0;
#define CHECK(x) \
  do { if (!(x)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); ++fails; } } while (0)

static constexpr uint64_t NWP = 4;
static constexpr int64_t NACT = 10;
static constexpr int WORLD = 3;
static constexpr int64_t GEN = 3;

static std::string slurp(const std::string& path) {
  const ckpt::File f = ckpt::open_file(path, "rb");
  std::string s;
  char buf[4096];
  size_t n;
  while (f && (n = std::fread(buf, 1, sizeof buf, f.get())) > 0) s.append(buf, n);
  return s;
}
static void spit(const std::string& path, const std::string& bytes) {
  const ckpt::File f = ckpt::open_file(path, "wb");
  CHECK(f && std::fwrite(bytes.data(), 1, bytes.size(), f.get()) == bytes.size());
}
static bool exists(const std::string& path) { struct stat st; return ::stat(path.c_str(), &st) == 0; }

// a search of 3 levels (1, 4, 6 states) over 3 ranks; rank 1 holds nothing of level 0 and 1
static const int64_t kGlobal[3] = {1, 4, 6};
static const int64_t kLocal[WORLD][3] = {{1, 3, 2}, {0, 0, 3}, {0, 1, 1}};

struct Fixture {
  std::string dir, path, desc;
  std::vector<int64_t> ag, ad;
  std::vector<ckpt::LevelRow> levels;
  ckpt::ShardHead mani;

  explicit Fixture(const std::string& d) : dir(d), path(d + "/s.ckpt"), desc(48, 'm') {
    for (int64_t k = 0; k < NACT; ++k) { ag.push_back(100 + k); ad.push_back(200 + k); }
    for (int l = 0; l < 3; ++l) levels.push_back({kGlobal[l], 10 * (l + 1)});
    mani = head(ckpt::kManifestMagic, -1, 11, 5, 6);
  }
  ckpt::ShardHead head(const char* magic, int64_t rank, uint64_t total, uint64_t lb, uint64_t lc) const {
    ckpt::ShardHead h;
    std::memset(&h, 0, sizeof h);
    std::memcpy(h.magic, magic, 8);
    h.nwp = NWP; h.total = total; h.level_begin = lb; h.level_count = lc; h.seed = 0x5EEDull;
    h.generated = 60; h.distinct = 11; h.depth = GEN; h.generated_in_model = 40; h.n_act = NACT; h.n_levels = 3;
    h.desc_len = (int64_t)desc.size(); h.fifo = 0; h.rank = rank; h.world = WORLD; h.generation = GEN;
    return h;
  }
  ckpt::ShardHead rank_head(int k) const {
    const uint64_t total = (uint64_t)(kLocal[k][0] + kLocal[k][1] + kLocal[k][2]);
    return head(ckpt::kRankMagic, k, total, total - (uint64_t)kLocal[k][2], (uint64_t)kLocal[k][2]);
  }
  std::vector<ckpt::LevelRow> rank_rows(int k) const {
    std::vector<ckpt::LevelRow> rows;
    for (int l = 0; l < 3; ++l) rows.push_back({kLocal[k][l], kGlobal[l]});
    return rows;
  }
  int write_rank(int k, const ckpt::ShardHead& h, const std::vector<ckpt::LevelRow>& rows, std::string& err) const {
    return ckpt::write_file(ckpt::rank_path(path, h.generation, k), h, desc, ag, ad, rows, [&](FILE* f) {
      std::vector<uint32_t> st(h.total * NWP, 0xA0000000u + (uint32_t)k);
      std::vector<uint64_t> me(h.total, ~0ull);
      return std::fwrite(st.data(), 4, st.size(), f) == st.size() && std::fwrite(me.data(), 8, me.size(), f) == me.size();
    }, err);
  }
  int write_manifest(const ckpt::ShardHead& h, std::string& err) const {
    return ckpt::write_file(path, h, desc, ag, ad, levels, [](FILE*) { return true; }, err);
  }
  void write_all() const {
    std::string err;
    for (int k = 0; k < WORLD; ++k) CHECK(write_rank(k, rank_head(k), rank_rows(k), err) == 0);
    CHECK(write_manifest(mani, err) == 0);
  }
  int open(ckpt::ShardSource& s, std::string& err) const { return ckpt::open_source(path, NWP, NACT, desc, s, err); }
  int open(std::string& err) const { ckpt::ShardSource s; return open(s, err); }
};

static void round_trip(const Fixture& fx) {
  std::string err;
  fx.write_all();
  CHECK(!exists(fx.path + ".tmp"));
  for (int k = 0; k < WORLD; ++k) CHECK(exists(ckpt::rank_path(fx.path, GEN, k)) && !exists(ckpt::rank_path(fx.path, GEN, k) + ".tmp"));
  CHECK(ckpt::rank_path("x", 12, 3) == "x.g12.r3");
  CHECK(ckpt::file_magic(fx.path) == ckpt::kManifestMagic && ckpt::file_magic(ckpt::rank_path(fx.path, GEN, 1)) == ckpt::kRankMagic);
  const std::string bytes = slurp(fx.path);
  CHECK(bytes.size() == 136 + 48 + 2 * 8 * (size_t)NACT + 3 * 16);
  CHECK(std::memcmp(bytes.data(), &fx.mani, 136) == 0);
  ckpt::ShardSource s;
  CHECK(fx.open(s, err) == 0 && err.empty());
  CHECK(s.world == WORLD && s.sharded && s.seed == 0x5EEDull && s.fifo == 0 && s.generated == 60 && s.distinct == 11 && s.depth == GEN &&
        s.generated_in_model == 40 && s.generation == GEN);
  CHECK(s.act_generated == fx.ag && s.act_distinct == fx.ad && s.levels.size() == 3 && s.parts.size() == (size_t)WORLD);
  for (size_t l = 0; l < s.levels.size() && l < 3; ++l) CHECK(s.levels[l].states == kGlobal[l] && s.levels[l].generated == 10 * ((int64_t)l + 1));
  for (int k = 0; k < WORLD && k < (int)s.parts.size(); ++k) {
    const ckpt::SourcePart& p = s.parts[k];
    CHECK(p.path == ckpt::rank_path(fx.path, GEN, k) && p.body == 136 + 48 + 2 * 8 * (uint64_t)NACT + 3 * 16);
    CHECK(p.total == (uint64_t)(kLocal[k][0] + kLocal[k][1] + kLocal[k][2]) && p.level_count.size() == 3);
    for (size_t l = 0; l < p.level_count.size() && l < 3; ++l) CHECK(p.level_count[l] == (uint64_t)kLocal[k][l]);
  }
}

static void manifest_cut(const Fixture& fx) {
  std::string err;
  fx.write_all();
  const std::string bytes = slurp(fx.path);
  for (size_t n = 0; n < bytes.size(); ++n) {
    spit(fx.path, bytes.substr(0, n));
    err.clear();
    const int rc = fx.open(err);
    if (n < 136 + 48) CHECK(rc == MC_E_INVALID);   // (below 8 bytes it is no manifest: refused as no single-GPU file either)
    else CHECK(rc == MC_E_IO && err == "checkpoint " + fx.path + " is truncated");
  }
  spit(fx.path, bytes + "x");   // bytes behind the level table
  CHECK(fx.open(err) == MC_E_INVALID);
  spit(fx.path, bytes);
  CHECK(fx.open(err) == 0);
}

static void bad_files(const Fixture& fx) {
  std::string err;
  auto refused = [&](const char* what, int want) {
    err.clear();
    const int rc = fx.open(err);
    if (rc != want) { std::fprintf(stderr, "%s: rc %d \"%s\", expected %d\n", what, rc, err.c_str(), want); ++fails; }
  };
  // the manifest's own fields
  fx.write_all();
  { ckpt::ShardHead h = fx.mani; h.world = 9; CHECK(fx.write_manifest(h, err) == 0); refused("manifest world 9", MC_E_INVALID); }
  { ckpt::ShardHead h = fx.mani; h.world = 0; CHECK(fx.write_manifest(h, err) == 0); refused("manifest world 0", MC_E_INVALID); }
  { ckpt::ShardHead h = fx.mani; h.total = 12; CHECK(fx.write_manifest(h, err) == 0); refused("manifest total", MC_E_INVALID); }
  { ckpt::ShardHead h = fx.mani; h.fifo = 1; CHECK(fx.write_manifest(h, err) == 0); refused("manifest fifo", MC_E_INVALID); }
  // a manifest of another world or generation than the rank files
  { ckpt::ShardHead h = fx.mani; h.world = 2; CHECK(fx.write_manifest(h, err) == 0); refused("world 2 over files of 3", MC_E_INVALID); }
  {
    ckpt::ShardHead h = fx.mani; h.generation = 4; h.depth = 4;
    CHECK(fx.write_manifest(h, err) == 0);
    refused("generation 4: its rank files are missing", MC_E_INVALID);
  }
  fx.write_all();
  refused("intact again", 0);
  // rank files: wrong rank, world, generation, seed
  for (int field = 0; field < 4; ++field) {
    ckpt::ShardHead h = fx.rank_head(1);
    if (field == 0) h.rank = 2;
    if (field == 1) h.world = 4;
    if (field == 2) h.generation = 2;
    if (field == 3) h.seed ^= 1;
    // (written under the name the manifest asks for)
    CHECK(ckpt::write_file(ckpt::rank_path(fx.path, GEN, 1), h, fx.desc, fx.ag, fx.ad, fx.rank_rows(1), [&](FILE* f) {
      std::vector<char> body(h.total * (NWP * 4 + 8), 0);
      return std::fwrite(body.data(), 1, body.size(), f) == body.size();
    }, err) == 0);
    refused(field == 0 ? "wrong rank" : field == 1 ? "wrong world" : field == 2 ? "wrong generation" : "wrong seed", MC_E_INVALID);
  }
  fx.write_all();
  // a rank file of another model
  {
    Fixture other(fx.dir);
    other.desc[3] ^= 1;
    CHECK(other.write_rank(2, other.rank_head(2), other.rank_rows(2), err) == 0);
    refused("rank file of another model", MC_E_INVALID);
  }
  fx.write_all();
  // level tables: a rank's global column differs; the ranks' rows do not sum to the manifest's
  { auto rows = fx.rank_rows(0); rows[1].generated = 5; CHECK(fx.write_rank(0, fx.rank_head(0), rows, err) == 0); refused("global column", MC_E_INVALID); }
  {
    auto rows = fx.rank_rows(0); rows[1].states = 2; rows[2].states = 3;   // the same total, one state moved to the next level
    ckpt::ShardHead h = fx.rank_head(0);
    h.level_count = 3; h.level_begin = 3;   // (the file agrees with itself)
    CHECK(fx.write_rank(0, h, rows, err) == 0);
    refused("rows do not sum to the manifest's levels", MC_E_INVALID);
    CHECK(err.find("level tables disagree") != std::string::npos);
  }
  { auto rows = fx.rank_rows(0); rows[2].states = 7; CHECK(fx.write_rank(0, fx.rank_head(0), rows, err) == 0); refused("row above the level", MC_E_INVALID); }
  { ckpt::ShardHead h = fx.rank_head(0); h.total += 1; CHECK(fx.write_rank(0, h, fx.rank_rows(0), err) == 0); refused("total != rows", MC_E_INVALID); }
  fx.write_all();
  // a rank file cut short (at every length: header + description INVALID, the rest IO), or with bytes behind its end
  {
    const std::string rp = ckpt::rank_path(fx.path, GEN, 0), bytes = slurp(rp);
    for (size_t n = 0; n < bytes.size(); ++n) {
      spit(rp, bytes.substr(0, n));
      err.clear();
      const int rc = fx.open(err);
      if (n < 136 + 48) CHECK(rc == MC_E_INVALID);
      else CHECK(rc == MC_E_IO && err == "checkpoint " + rp + " is truncated");
    }
    spit(rp, bytes + "x");
    refused("rank file too long", MC_E_INVALID);
    spit(rp, bytes);
    refused("intact again", 0);
  }
  // a missing rank file
  ::unlink(ckpt::rank_path(fx.path, GEN, 1).c_str());
  refused("missing rank file", MC_E_INVALID);
  CHECK(err.find("is missing") != std::string::npos);
  // no file at all
  ::unlink(fx.path.c_str());
  refused("no manifest", MC_E_IO);
}

// what the writer removes once a new manifest is in place
static void stale_files(const Fixture& fx) {
  fx.write_all();
  ckpt::remove_stale_rank_files(fx.path, GEN, WORLD, GEN, WORLD);   // the same generation: nothing goes
  for (int k = 0; k < WORLD; ++k) CHECK(exists(ckpt::rank_path(fx.path, GEN, k)));
  ckpt::remove_stale_rank_files(fx.path, GEN, WORLD, GEN, 2);       // ... at a smaller world: the ranks behind it
  CHECK(exists(ckpt::rank_path(fx.path, GEN, 1)) && !exists(ckpt::rank_path(fx.path, GEN, 2)));
  ckpt::remove_stale_rank_files(fx.path, GEN, WORLD, GEN + 1, WORLD);
  for (int k = 0; k < WORLD; ++k) CHECK(!exists(ckpt::rank_path(fx.path, GEN, k)));
  ::unlink(fx.path.c_str());
}

// a single-GPU RAFTMCK2 file is a source of one part, in either search order
static void single_file(const Fixture& fx) {
  std::string err;
  for (int64_t fifo = 0; fifo < 2; ++fifo) {
    ckpt::OrigHead h;
    std::memset(&h, 0, sizeof h);
    std::memcpy(h.magic, ckpt::kOrigMagic, 8);
    h.nwp = NWP; h.total = 11; h.level_begin = 5; h.level_count = 6; h.seed = 7; h.generated = 60; h.distinct = 11; h.depth = 3;
    h.generated_in_model = 40; h.n_act = NACT; h.n_levels = 3; h.desc_len = (int64_t)fx.desc.size(); h.fifo = fifo;
    auto write = [&](const ckpt::OrigHead& hh, size_t body) {
      return ckpt::write_file(fx.path, hh, fx.desc, fx.ag, fx.ad, fx.levels, [&](FILE* f) {
        std::vector<char> b(body, 0);
        return std::fwrite(b.data(), 1, b.size(), f) == b.size();
      }, err);
    };
    CHECK(write(h, 11 * (NWP * 4 + 8)) == 0);
    ckpt::ShardSource s;
    CHECK(fx.open(s, err) == 0 && s.world == 1 && !s.sharded && s.fifo == fifo && s.seed == 7 && s.parts.size() == 1 && s.generation == 3);
    if (s.parts.size() == 1) {
      CHECK(s.parts[0].path == fx.path && s.parts[0].total == 11 && s.parts[0].body == 112 + 48 + 2 * 8 * (uint64_t)NACT + 3 * 16);
      CHECK(s.parts[0].level_count == std::vector<uint64_t>({1, 4, 6}));
    }
    CHECK(write(h, 11 * (NWP * 4 + 8) - 1) == 0 && fx.open(err) == MC_E_IO);
    CHECK(write(h, 11 * (NWP * 4 + 8) + 1) == 0 && fx.open(err) == MC_E_INVALID);
    { ckpt::OrigHead b = h; b.total = 12; b.distinct = 12; CHECK(write(b, 12 * (NWP * 4 + 8)) == 0 && fx.open(err) == MC_E_INVALID); }   // levels sum to 11
    { ckpt::OrigHead b = h; b.level_begin = 4; CHECK(write(b, 11 * (NWP * 4 + 8)) == 0 && fx.open(err) == MC_E_INVALID); }
    { ckpt::OrigHead b = h; b.fifo = 2; CHECK(write(b, 11 * (NWP * 4 + 8)) == 0 && fx.open(err) == MC_E_INVALID); }
  }
  ::unlink(fx.path.c_str());
}

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: shard_ckpt_check DIR\n"); return 2; }
  const Fixture fx(argv[1]);
  round_trip(fx);
  manifest_cut(fx);
  bad_files(fx);
  stale_files(fx);
  single_file(fx);
  if (fails) { std::fprintf(stderr, "%d check(s) failed\n", fails); return 1; }
  std::printf("ok\n");
  return 0;
}
