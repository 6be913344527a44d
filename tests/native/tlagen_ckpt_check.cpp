// The generated path's checkpoint file (csrc/ckpt_file.h: GenHead, check_gen_head, read_gen_body) on
// the host: a round trip of header and body, the file cut at every length, the refused headers, a
// write that cannot be made, and crafted bodies that must be refused before anything is indexed with
// their values.  Built with -fsanitize=address,undefined and run directly
// (tests/test_tlagen_ckpt_file.py); the load is the backend's own, with host vectors where the
// backend has device arrays.
//   tlagen_ckpt_check DIR     (an empty scratch directory)      prints "ok" and exits 0, or says what failed
#include <sys/stat.h>
#include <unistd.h>

#include <cstdlib>

#include "ckpt_file.h"

using namespace rmc;

static int fails = 0;
#define CHECK(x) \
  do { if (!(x)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); ++fails; } } while (0)

struct Level { int64_t states, generated; };
static constexpr int64_t NACT = 3;
static const char* const MAGIC = "RAFTMCG1";

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

// a store of variable-width states: 3 levels (1, 2, 3 states), state i of 2 + i words
struct Store {
  std::vector<uint64_t> offs, parent;
  std::vector<uint32_t> act, words;
  bool operator==(const Store& o) const { return offs == o.offs && parent == o.parent && act == o.act && words == o.words; }
};
struct Model {
  ckpt::GenHead h;
  std::string desc = "tlagen 0123456789abcdef variables x y actions A B C";
  std::vector<int64_t> act_generated{5, 6, 7}, act_distinct{1, 2, 2};
  std::vector<Level> levels{{1, 1}, {2, 7}, {3, 10}};
  Store s;
  Model() {
    for (uint64_t i = 0; i < 6; ++i) {
      s.offs.push_back(s.words.size());
      s.parent.push_back(i == 0 ? ~0ull : (i - 1) / 2);
      s.act.push_back((uint32_t)(i % 3));
      for (uint64_t q = 0; q < 2 + i; ++q) s.words.push_back((uint32_t)(0xB0000000u + 16 * i + q));
    }
    std::memset(&h, 0, sizeof h);
    std::memcpy(h.magic, MAGIC, 8);
    h.nwp = 0; h.total = 6; h.level_begin = 3; h.level_count = 3; h.seed = 0x5EEDull; h.words = s.words.size(); h.fifo = 1;
    h.generated = 18; h.distinct = 6; h.depth = 3; h.generated_in_model = 12; h.n_act = NACT; h.n_levels = 3; h.desc_len = (int64_t)desc.size();
  }
  size_t head_bytes() const { return sizeof h + desc.size() + 2 * 8 * (size_t)NACT + 3 * 16; }
  int write(const std::string& path, std::string& err) const { return write(path, h, s, err); }
  int write(const std::string& path, const ckpt::GenHead& hh, const Store& st, std::string& err) const {
    return ckpt::write_file(path, hh, desc, act_generated, act_distinct, levels, [&](FILE* f) {
      return std::fwrite(st.offs.data(), 8, st.offs.size(), f) == st.offs.size() && std::fwrite(st.parent.data(), 8, st.parent.size(), f) == st.parent.size() &&
             std::fwrite(st.act.data(), 4, st.act.size(), f) == st.act.size() && std::fwrite(st.words.data(), 4, st.words.size(), f) == st.words.size();
    }, err);
  }
  // the whole file as a recovery reads it (chunks of `chunk` bytes): 0, or the reader's error
  int read(const std::string& path, size_t chunk, ckpt::GenHead& h2, std::vector<Level>& lv, Store& out, std::string& err) const {
    ckpt::Reader in(path);
    std::vector<int64_t> ag, ad;
    if (int rc = in.head(MAGIC, 0, NACT, desc, h2, ag, ad, lv, err)) return rc;
    if (int rc = ckpt::check_gen_head(in, h2, lv, err)) return rc;
    if (ag != act_generated || ad != act_distinct) { err = "counters differ"; return -100; }
    // (only now are the arrays sized by the header: check_gen_head has tied total and words to the file's length)
    out.offs.assign(h2.total, 0); out.parent.assign(h2.total, 0); out.act.assign(h2.total, 0); out.words.assign(h2.words, 0);
    return ckpt::read_gen_body(in, h2, (uint64_t)lv.front().states, chunk, [&](int kind, const void* data, uint64_t first, uint64_t n, std::string&) -> int {
      void* dst = kind == 0 ? (void*)(out.offs.data() + first) : kind == 1 ? (void*)(out.parent.data() + first)
                : kind == 2 ? (void*)(out.act.data() + first) : (void*)(out.words.data() + first);
      std::memcpy(dst, data, n * (kind < 2 ? 8 : 4));
      return 0;
    }, err);
  }
  int read(const std::string& path, std::string& err) const {
    ckpt::GenHead h2; std::vector<Level> lv; Store out;
    const int rc = read(path, 16, h2, lv, out, err);
    if (rc == 0)   // what a recovery does next: every state's words, through its offset
      for (uint64_t i = 0; i < h2.total; ++i) {
        const uint64_t end = i + 1 < h2.total ? out.offs[i + 1] : h2.words;
        uint32_t x = 0;
        for (uint64_t q = out.offs[i]; q < end; ++q) x ^= out.words[q];
        if (out.parent[i] != ~0ull) x ^= out.act[out.parent[i]];
        if (x == 0x12345678u) std::fprintf(stderr, "(unlikely)\n");
      }
    return rc;
  }
};

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: tlagen_ckpt_check DIR\n"); return 2; }
  const std::string dir = argv[1], path = dir + "/gen.ckpt", cut = dir + "/cut.ckpt";
  const Model m;
  std::string err;
  const std::string invalid = "checkpoint " + cut + " is not a checkpoint of this model", truncated = "checkpoint " + cut + " is truncated";
  // round trip, whole and in chunks of 8 and 24 bytes
  CHECK(m.write(path, err) == 0 && err.empty());
  CHECK(!exists(path + ".tmp"));
  const std::string bytes = slurp(path);
  CHECK(bytes.size() == m.head_bytes() + 6 * 20 + m.s.words.size() * 4);
  CHECK(sizeof(ckpt::GenHead) == 120 && std::memcmp(bytes.data(), &m.h, 120) == 0);   // the header goes to disk as it lies in memory
  for (size_t chunk : {size_t(1) << 20, size_t(8), size_t(24)}) {
    ckpt::GenHead h2; std::vector<Level> lv; Store out;
    CHECK(m.read(path, chunk, h2, lv, out, err) == 0);
    CHECK(std::memcmp(&h2, &m.h, sizeof h2) == 0 && out == m.s && lv.size() == 3);
    for (size_t k = 0; k < lv.size() && k < 3; ++k) CHECK(lv[k].states == m.levels[k].states && lv[k].generated == m.levels[k].generated);
  }
  // cut at every length: inside header + description no checkpoint of this model, behind them truncated
  for (size_t n = 0; n < bytes.size(); ++n) {
    spit(cut, bytes.substr(0, n));
    err.clear();
    const int rc = m.read(cut, err);
    if (n < 120 + m.desc.size()) CHECK(rc == MC_E_INVALID && err == invalid);
    else CHECK(rc == MC_E_IO && err == truncated);
  }
  { spit(cut, bytes + std::string(4, '\0')); err.clear(); CHECK(m.read(cut, err) == MC_E_INVALID && err == invalid); }   // longer than its header says
  // refused headers
  auto refused = [&](const char* what, const ckpt::GenHead& bad) {
    std::string b = bytes;
    std::memcpy(&b[0], &bad, sizeof bad);
    spit(cut, b);
    err.clear();
    const int rc = m.read(cut, err);
    if (!(rc == MC_E_INVALID && err == invalid)) { std::fprintf(stderr, "%s: rc %d \"%s\"\n", what, rc, err.c_str()); ++fails; }
  };
  { ckpt::GenHead bad = m.h; std::memcpy(bad.magic, "RAFTMCK2", 8); refused("another family's magic", bad); }
  { ckpt::GenHead bad = m.h; bad.n_act += 1; refused("wrong n_act", bad); }
  { ckpt::GenHead bad = m.h; bad.desc_len = 1 << 20; refused("desc_len 2^20", bad); }
  { ckpt::GenHead bad = m.h; bad.nwp = 4; refused("a fixed state width", bad); }
  { ckpt::GenHead bad = m.h; bad.level_begin = 2; refused("level_begin + level_count != total", bad); }
  { ckpt::GenHead bad = m.h; bad.level_count = 2; bad.level_begin = 4; refused("level_count not the last level's", bad); }
  { ckpt::GenHead bad = m.h; bad.depth = 4; refused("depth != n_levels", bad); }
  { ckpt::GenHead bad = m.h; bad.fifo = 2; refused("fifo 2", bad); }
  { ckpt::GenHead bad = m.h; bad.total = 7; bad.distinct = 7; refused("total not the levels' sum", bad); }
  { ckpt::GenHead bad = m.h; bad.words = 2; refused("fewer words than states", bad); }
  { std::string b = bytes; b[120 + 5] ^= 1; spit(cut, b); CHECK(m.read(cut, err) == MC_E_INVALID); }   // another model's description
  CHECK(m.read(dir + "/absent.ckpt", err) == MC_E_IO && err == "cannot read checkpoint " + dir + "/absent.ckpt");
  // `total` beyond the file: no array is sized by it, the length check refuses first
  {
    std::string b = bytes;
    ckpt::GenHead bad = m.h; bad.total = (1ull << 39); bad.distinct = (int64_t)bad.total; bad.level_count = bad.total - 3; bad.words = bad.total;
    std::memcpy(&b[0], &bad, sizeof bad);
    const int64_t st = (int64_t)bad.level_count;
    std::memcpy(&b[120 + m.desc.size() + 2 * 8 * NACT + 2 * 16], &st, 8);   // the last level's states, so the levels add up
    spit(cut, b); err.clear();
    CHECK(m.read(cut, err) == MC_E_IO && err == truncated);
  }
  // crafted bodies (header and length consistent): refused before any indexing
  auto crafted = [&](const char* what, const Store& st) {
    err.clear();
    CHECK(m.write(cut, m.h, st, err) == 0);
    err.clear();
    const int rc = m.read(cut, err);
    if (!(rc == MC_E_INVALID && err == invalid)) { std::fprintf(stderr, "%s: rc %d \"%s\"\n", what, rc, err.c_str()); ++fails; }
  };
  { Store st = m.s; st.offs[4] = m.h.words; crafted("offs[i] == words", st); }
  { Store st = m.s; st.offs[5] = 1ull << 40; crafted("offs[i] far past words", st); }
  { Store st = m.s; st.offs[0] = 1; crafted("offs[0] != 0", st); }
  { Store st = m.s; st.offs[3] = st.offs[2]; crafted("offs not ascending", st); }
  { Store st = m.s; st.parent[4] = 4; crafted("parent[i] == i", st); }
  { Store st = m.s; st.parent[2] = 5; crafted("parent[i] > i", st); }
  { Store st = m.s; st.parent[3] = ~0ull; crafted("a non-initial state without a parent", st); }
  { Store st = m.s; st.parent[0] = 0; crafted("an initial state with a parent", st); }
  // a write that cannot be made: no file at the final path; one that fails half way keeps the old file
  err.clear();
  const std::string nodir = dir + "/no_such_dir/x.ckpt";
  CHECK(m.write(nodir, err) == MC_E_IO && err == "cannot write checkpoint " + nodir + ".tmp" && !exists(nodir));
  err.clear();
  const std::string fresh = dir + "/fresh.ckpt";
  CHECK(ckpt::write_file(fresh, m.h, m.desc, m.act_generated, m.act_distinct, m.levels, [](FILE*) { return false; }, err) == MC_E_IO && !exists(fresh));
  CHECK(ckpt::write_file(path, m.h, m.desc, m.act_generated, m.act_distinct, m.levels, [](FILE*) { return false; }, err) == MC_E_IO &&
        err == "writing checkpoint " + path + " failed");
  CHECK(slurp(path) == bytes);
  ::unlink((path + ".tmp").c_str());
  ::unlink((fresh + ".tmp").c_str());
  ::unlink(path.c_str());
  ::unlink(cut.c_str());
  if (fails) { std::fprintf(stderr, "%d check(s) failed\n", fails); return 1; }
  std::printf("ok\n");
  return 0;
}
