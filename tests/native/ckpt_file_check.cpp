// The checkpoint framing (csrc/ckpt_file.h) on the host, for both family headers: a round trip, the
// file cut at every length, the refused headers and a write that cannot be made.  Built with
// -fsanitize=address,undefined and run directly (tests/test_ckpt_file.py); the body of the file is a
// host-only store (csrc/host_store.h), as a checkpoint whose states were all spilled.
//   ckpt_file_check DIR     (an empty scratch directory)      prints "ok" and exits 0, or says what failed
#include <sys/stat.h>
#include <unistd.h>

#include <cstdlib>

#include "ckpt_file.h"
#include "host_store.h"

using namespace rmc;

static int fails = 0;
#define CHECK(x) \
  do { if (!(x)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); ++fails; } } while (0)

static constexpr int NWP = 4;
static constexpr uint64_t NST = 5;   // stored states
struct Level { int64_t states, generated; };
struct Counters { std::vector<int64_t> act_generated, act_distinct; std::vector<Level> levels; };

static bool same_head(const ckpt::OrigHead& a, const ckpt::OrigHead& b) { return std::memcmp(&a, &b, sizeof a) == 0; }
static bool same_head(const ckpt::MembHead& a, const ckpt::MembHead& b) { return std::memcmp(&a, &b, sizeof a) == 0; }
static void family_word(ckpt::OrigHead& h) { h.fifo = 1; }
static void family_word(ckpt::MembHead& h) { h.sym_tlc = 1; }

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

template <class H>
struct Case {
  const char* magic;
  int64_t n_act;
  H h;
  std::string desc;
  Counters c;
  HostStore store{NWP};

  Case(const char* m, int64_t na) : magic(m), n_act(na) {
    desc = std::string(64, 'd');
    for (int k = 0; k < 64; ++k) desc[k] = (char)('!' + k);
    std::memset(&h, 0, sizeof h);
    std::memcpy(h.magic, magic, 8);
    h.nwp = NWP; h.total = NST; h.level_begin = 3; h.level_count = 2; h.seed = 0x5EEDull;
    h.generated = 17; h.distinct = (int64_t)NST; h.depth = 3; h.generated_in_model = 11;
    h.n_act = na; h.n_levels = 3; h.desc_len = (int64_t)desc.size();
    family_word(h);
    for (int64_t k = 0; k < na; ++k) { c.act_generated.push_back(100 + k); c.act_distinct.push_back(200 + k); }
    c.levels = {{1, 2}, {2, 9}, {2, 6}};
    uint32_t* st = nullptr; uint64_t* me = nullptr;
    store.append(NST, &st, &me);
    for (uint64_t k = 0; k < NST * NWP; ++k) st[k] = (uint32_t)(0xA0000000u + k);
    for (uint64_t k = 0; k < NST; ++k) me[k] = k ? ((k - 1) << 24) | (3u << 16) : ~0ull;
  }
  int write(const std::string& path, std::string& err) const {
    return ckpt::write_file(path, h, desc, c.act_generated, c.act_distinct, c.levels,
                            [&](FILE* f) { return store.write_states(f) && store.write_meta(f); }, err);
  }
  // the whole file as a recovery reads it: 0, or the reader's error
  int read(const std::string& path, H& h2, Counters& c2, std::vector<uint32_t>& st, std::vector<uint64_t>& me, std::string& err) const {
    ckpt::Reader in(path);
    if (int rc = in.head(magic, NWP, n_act, desc, h2, c2.act_generated, c2.act_distinct, c2.levels, err)) return rc;
    st.assign(h2.total * NWP, 0); me.assign(h2.total, 0);
    if (std::fread(st.data(), 4, st.size(), in.file()) != st.size() || std::fread(me.data(), 8, me.size(), in.file()) != me.size())
      return in.truncated(err);
    return 0;
  }
  int read(const std::string& path, std::string& err) const {
    H h2; Counters c2; std::vector<uint32_t> st; std::vector<uint64_t> me;
    return read(path, h2, c2, st, me, err);
  }

  void run(const std::string& dir) {
    const std::string path = dir + "/" + magic + ".ckpt", cut = dir + "/cut.ckpt";
    std::string err;
    // round trip
    CHECK(write(path, err) == 0 && err.empty());
    CHECK(!exists(path + ".tmp"));
    const std::string bytes = slurp(path);
    CHECK(bytes.size() == 112 + 64 + 2 * 8 * (size_t)n_act + 3 * 16 + NST * (NWP * 4 + 8));
    CHECK(std::memcmp(bytes.data(), &h, 112) == 0);   // the header goes to disk as it lies in memory
    {
      H h2; Counters c2; std::vector<uint32_t> st; std::vector<uint64_t> me;
      CHECK(read(path, h2, c2, st, me, err) == 0);
      CHECK(same_head(h, h2));
      CHECK(c2.act_generated == c.act_generated && c2.act_distinct == c.act_distinct && c2.levels.size() == 3);
      for (size_t k = 0; k < c2.levels.size() && k < 3; ++k)
        CHECK(c2.levels[k].states == c.levels[k].states && c2.levels[k].generated == c.levels[k].generated);
      CHECK(st.size() == NST * NWP && std::memcmp(st.data(), store.state(0), st.size() * 4) == 0);
      for (uint64_t k = 0; k < NST && k < me.size(); ++k) CHECK(me[k] == store.meta(k));
    }
    // cut at every length: before the end of the description it is no checkpoint of this model, behind it truncated
    for (size_t n = 0; n < bytes.size(); ++n) {
      spit(cut, bytes.substr(0, n));
      err.clear();
      const int rc = read(cut, err);
      if (n < 112 + 64) CHECK(rc == MC_E_INVALID && err == "checkpoint " + cut + " is not a checkpoint of this model");
      else CHECK(rc == MC_E_IO && err == "checkpoint " + cut + " is truncated");
    }
    // refused headers
    auto refused = [&](const char* what, H bad) {
      std::string b = bytes;
      std::memcpy(&b[0], &bad, sizeof bad);
      spit(cut, b);
      err.clear();
      const int rc = read(cut, err);
      if (!(rc == MC_E_INVALID && err == "checkpoint " + cut + " is not a checkpoint of this model")) {
        std::fprintf(stderr, "%s %s: rc %d \"%s\"\n", magic, what, rc, err.c_str());
        ++fails;
      }
    };
    { H bad = h; bad.magic[7] ^= 1; refused("wrong magic", bad); }
    { H bad = h; bad.desc_len = 1 << 20; refused("desc_len 2^20", bad); }
    { H bad = h; bad.desc_len = -1; refused("desc_len -1", bad); }
    { H bad = h; bad.n_levels = 0; refused("n_levels 0", bad); }
    { H bad = h; bad.n_levels = 1 << 20; refused("n_levels 2^20", bad); }
    { H bad = h; bad.n_act += 1; refused("wrong n_act", bad); }
    { H bad = h; bad.nwp += 4; refused("wrong nwp", bad); }
    { std::string b = bytes; b[112 + 5] ^= 1; spit(cut, b); CHECK(read(cut, err) == MC_E_INVALID); }   // another model's description
    CHECK(read(dir + "/absent.ckpt", err) == MC_E_IO && err == "cannot read checkpoint " + dir + "/absent.ckpt");
    // a write that cannot be made: no file at the final path
    err.clear();
    const std::string nodir = dir + "/no_such_dir/x.ckpt";
    CHECK(write(nodir, err) == MC_E_IO && err == "cannot write checkpoint " + nodir + ".tmp" && !exists(nodir));
    const std::string ro = dir + "/ro";
    CHECK(::mkdir(ro.c_str(), 0555) == 0);
    if (::access(ro.c_str(), W_OK) != 0) {   // (root writes anywhere: the missing directory above is its case)
      err.clear();
      CHECK(write(ro + "/x.ckpt", err) == MC_E_IO && !exists(ro + "/x.ckpt"));
    }
    ::rmdir(ro.c_str());
    // ... and one that fails half way (the body): the checkpoint that was there stays as it was
    err.clear();
    CHECK(ckpt::write_file(path, h, desc, c.act_generated, c.act_distinct, c.levels, [](FILE*) { return false; }, err) == MC_E_IO && err == "writing checkpoint " + path + " failed");
    CHECK(slurp(path) == bytes);
    ::unlink((path + ".tmp").c_str());
    ::unlink(path.c_str());
    ::unlink(cut.c_str());
  }
};

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: ckpt_file_check DIR\n"); return 2; }
  Case<ckpt::OrigHead>("RAFTMCK2", 10).run(argv[1]);
  Case<ckpt::MembHead>("RAFTMCM1", 17).run(argv[1]);
  if (fails) { std::fprintf(stderr, "%d check(s) failed\n", fails); return 1; }
  std::printf("ok\n");
  return 0;
}
