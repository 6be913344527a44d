// TEST HARNESS ONLY (never part of the product).  tlc_membership's seen-set stage, run as the product
// runs it -- memb_dedup_cells, memb_select, memb_scan_blocks, memb_compact -- on synthetic, seeded,
// adversarial cell lists, and memb_scan_blocks alone at its block-count edges, each checked against a
// plain sequential model.  The backend translation unit is included as it stands, so the kernels are
// the product's own text.
//   memb_seen_set_check [--host-only]   -> one JSON line per case (seen_set_check.h: Report)
// --host-only makes no HIP call: the outputs come from a sequential host routine that plays the four
// kernels, go through the same check functions, and are then perturbed to show that the checks can fail.
#include "../../raft-tla_amd/csrc/memb_backend.hip"

#include "seen_set_check.h"

using namespace rmc;
using ssc::fmt;
using ssc::Report;
using ssc::Rng;

static bool g_host_only = false;
static const u64 JUNK = 0xEEEEEEEEEEEEEEEEull;

struct PipeIn {
  u64 chunk_count = 0, chunk_begin = 0, rank0 = 0, nslot = 0, level = 0, slots = 0;
  u32 smw = 0;
  std::vector<u64> cand;         // [nslot][chunk] fingerprints of the in-model cells (0 elsewhere)
  std::vector<u32> cells;        // per workgroup BS * nslot, four wave regions
  std::vector<u32> cell_count;   // per workgroup 8 (the first four: in-model cells per wave)
  std::vector<u64> smask;        // [smw][chunk]
  std::vector<u64> table;        // {fp, ~(level << 40 | key)}
  u32 nblk() const { return (u32)((chunk_count + BS - 1) / BS); }
};
struct PipeOut {
  std::vector<u64> table, cand, newrec;
  std::vector<unsigned int> woff;
  std::vector<unsigned long long> bsum;
  u64 c_new = 0, err = 0;
};

// the in-model cells in key order (state-major, then slot): what smask says
static std::vector<u32> cells_in_key_order(const PipeIn& in) {
  std::vector<u32> v;
  for (u64 st = 0; st < in.chunk_count; ++st)
    for (u64 sl = 0; sl < in.nslot; ++sl)
      if ((in.smask[(sl / 64) * in.chunk_count + st] >> (sl % 64)) & 1) v.push_back((u32)(sl * in.chunk_count + st));
  return v;
}
static u64 cell_key(const PipeIn& in, u32 cell) {
  const u64 sl = cell / in.chunk_count, st = cell - sl * in.chunk_count;
  return (in.rank0 + st) * in.nslot + sl;
}
static u64 cell_rec(const PipeIn& in, u32 cell) {
  const u64 sl = cell / in.chunk_count, st = cell - sl * in.chunk_count;
  return ((in.chunk_begin + st) << 10) | sl;
}

// the cell lists, the masks and the fingerprints must describe the same cells before a kernel reads them
static void validate(const PipeIn& in) {
  std::multiset<u32> listed, masked;
  for (u32 b = 0; b < in.nblk(); ++b)
    for (u32 w = 0; w < 4; ++w) {
      const u32 c = in.cell_count[8 * b + w];
      bool ok = c <= 64 * in.nslot;
      for (u32 i = 0; ok && i < c; ++i) {
        const u32 cell = in.cells[b * BS * in.nslot + w * 64 * in.nslot + i];
        ok = cell < in.nslot * in.chunk_count && (cell % in.chunk_count) / BS == b && in.cand[cell] != 0;
        listed.insert(cell);
      }
      if (!ok) { std::printf("{\"error\": \"bad case: cell list\"}\n"); std::exit(2); }
    }
  for (u32 c : cells_in_key_order(in)) masked.insert(c);
  if (listed != masked) { std::printf("{\"error\": \"bad case: cell lists and masks differ\"}\n"); std::exit(2); }
}

static PipeOut run_pipe(const PipeIn& in) {
  validate(in);
  const u32 nblk = in.nblk();
  ssc::DevBuf<u64> cand(in.cand), smask(in.smask), table(in.table), newrec(std::vector<u64>(in.nslot * in.chunk_count + 1, JUNK));
  ssc::DevBuf<u32> cells(in.cells), cell_count(in.cell_count);
  ssc::DevBuf<unsigned int> woff(std::vector<unsigned int>(in.chunk_count, 0xEEEEEEEEu));
  ssc::DevBuf<unsigned long long> bsum(std::vector<unsigned long long>(nblk, JUNK)), ctr(std::vector<unsigned long long>(C_NCTR, 0));
  MDedupArgs d{};
  d.cells = cells.p; d.cell_count = cell_count.p; d.cand = cand.p; d.nslots = in.slots; d.chunk_count = in.chunk_count; d.rank0 = in.rank0;
  d.nslot = in.nslot; d.level = in.level; d.table = table.p; d.table_mask = in.slots - 1; d.ctr = ctr.p;
  hipLaunchKernelGGL(memb_dedup_cells, dim3(nblk), dim3(BS), 0, 0, d);
  ssc::launched("memb_dedup_cells");
  MSelArgs s{};
  s.smask = smask.p; s.smw = in.smw; s.cand = cand.p; s.chunk_count = in.chunk_count; s.rank0 = in.rank0; s.nslot = in.nslot; s.level = in.level;
  s.table = table.p; s.woff = woff.p; s.bsum = bsum.p;
  hipLaunchKernelGGL(memb_select, dim3(nblk), dim3(BS), 0, 0, s);
  ssc::launched("memb_select");
  hipLaunchKernelGGL(memb_scan_blocks, dim3(1), dim3(BS), 0, 0, bsum.p, nblk, ctr.p);
  ssc::launched("memb_scan_blocks");
  MCompArgs c{};
  c.smask = smask.p; c.smw = in.smw; c.cand = cand.p; c.chunk_count = in.chunk_count; c.chunk_begin = in.chunk_begin; c.nslot = in.nslot;
  c.woff = woff.p; c.bsum = bsum.p; c.newrec = newrec.p;
  hipLaunchKernelGGL(memb_compact, dim3(nblk), dim3(BS), 0, 0, c);
  ssc::launched("memb_compact");
  PipeOut o;
  o.table = table.get(); o.cand = cand.get(); o.newrec = newrec.get(); o.woff = woff.get(); o.bsum = bsum.get();
  o.c_new = ctr.get()[C_NEW]; o.err = ctr.get()[C_ERR];
  o.newrec.resize(o.c_new < o.newrec.size() ? o.c_new : o.newrec.size());
  return o;
}

// the four kernels played sequentially, cell by cell
static PipeOut play_pipe(const PipeIn& in) {
  PipeOut o;
  o.table = in.table; o.cand = in.cand;
  const u64 mask = in.slots - 1;
  const std::vector<u32> order = cells_in_key_order(in);
  for (u32 cell : order) {
    const u64 fp = in.cand[cell], nk = ~((in.level << 40) | cell_key(in, cell));
    u64 s = fp & mask;
    while (o.table[2 * s] && o.table[2 * s] != fp) s = (s + 1) & mask;
    o.table[2 * s] = fp;
    if (o.table[2 * s + 1] < nk) o.table[2 * s + 1] = nk;
    o.cand[cell] = s + 1;
  }
  std::vector<unsigned int> per(in.chunk_count, 0);
  for (u32 cell : order)
    if (o.table[2 * (o.cand[cell] - 1) + 1] == ~((in.level << 40) | cell_key(in, cell))) {
      o.cand[cell] |= WINBIT;
      ++per[cell % in.chunk_count];
      o.newrec.push_back(cell_rec(in, cell));
    }
  o.woff.assign(in.chunk_count, 0); o.bsum.assign(in.nblk(), 0);
  u64 run = 0;
  for (u32 b = 0; b < in.nblk(); ++b) {
    o.bsum[b] = run;
    unsigned int local = 0;
    for (u64 st = (u64)b * BS; st < in.chunk_count && st < (u64)(b + 1) * BS; ++st) { o.woff[st] = local; local += per[st]; }
    run += local;
  }
  o.c_new = run;
  return o;
}

static std::string check_pipe(const PipeIn& in, const PipeOut& out) {
  const u64 mask = in.slots - 1;
  std::unordered_map<u64, u64> before, want;   // fp -> ~(level << 40 | key): the maximum complement is the first-found producer
  for (u64 s = 0; s <= mask; ++s) if (in.table[2 * s]) before[in.table[2 * s]] = in.table[2 * s + 1];
  want = before;
  const std::vector<u32> order = cells_in_key_order(in);
  for (u32 cell : order) {
    const u64 nk = ~((in.level << 40) | cell_key(in, cell));
    auto it = want.find(in.cand[cell]);
    if (it == want.end()) want[in.cand[cell]] = nk; else if (it->second < nk) it->second = nk;
  }
  if (out.err) return fmt("ctr[C_ERR] = %llx", (unsigned long long)out.err);
  // the table: every fingerprint once, with its minimum (level, key)
  std::set<u64> stored;
  for (u64 s = 0; s <= mask; ++s) {
    const u64 f = out.table[2 * s];
    if (!f) continue;
    auto it = want.find(f);
    if (it == want.end()) return fmt("slot %llu holds %016llx, which nobody gave", (unsigned long long)s, (unsigned long long)f);
    if (!stored.insert(f).second) return fmt("fingerprint %016llx is stored twice", (unsigned long long)f);
    if (out.table[2 * s + 1] != it->second) return fmt("fingerprint %016llx: key word %llx, minimum given %llx", (unsigned long long)f, (unsigned long long)~out.table[2 * s + 1], (unsigned long long)~it->second);
  }
  if (stored.size() != want.size()) return fmt("%zu fingerprints stored, %zu expected: a fingerprint was lost", stored.size(), want.size());
  // winners: the minimum-key producer of every fingerprint this chunk brought in or took over
  std::vector<u64> recs;
  std::vector<unsigned int> per(in.chunk_count, 0);
  for (u32 cell : order) {   // key order
    const u64 nk = ~((in.level << 40) | cell_key(in, cell));
    const bool wins = want[in.cand[cell]] == nk;
    const u64 c = out.cand[cell];
    if (((c & WINBIT) != 0) != wins) return fmt("cell %u (fingerprint %016llx): winner bit %d, model %d", cell, (unsigned long long)in.cand[cell], (int)((c & WINBIT) != 0), (int)wins);
    const u64 pos = (c & ~WINBIT) - 1;
    if (pos > mask || out.table[2 * pos] != in.cand[cell]) return fmt("cell %u: cand names entry %llu, which does not hold its fingerprint", cell, (unsigned long long)pos);
    if (wins) { recs.push_back(cell_rec(in, cell)); ++per[cell % in.chunk_count]; }
  }
  u64 fresh = 0;
  for (auto& w : want) { auto it = before.find(w.first); if (it == before.end() || it->second != w.second) ++fresh; }
  if (fresh != recs.size()) return "model: winners and new fingerprints differ";
  if (out.c_new != recs.size()) return fmt("ctr[C_NEW] = %llu, %zu fingerprints are new", (unsigned long long)out.c_new, recs.size());
  if (out.newrec.size() != recs.size()) return "fewer records than ctr[C_NEW]";
  for (size_t i = 0; i < recs.size(); ++i)
    if (out.newrec[i] != recs[i]) return fmt("newrec[%zu] = %llx, in key order %llx", i, (unsigned long long)out.newrec[i], (unsigned long long)recs[i]);
  std::vector<unsigned int> blk(in.nblk(), 0);
  for (u64 st = 0; st < in.chunk_count; ++st) {
    if (out.woff[st] != blk[st / BS]) return fmt("woff[%llu] = %u, serial scan %u", (unsigned long long)st, out.woff[st], blk[st / BS]);
    blk[st / BS] += per[st];
  }
  std::vector<unsigned long long> off;
  ssc::serial_scan(blk, off);
  for (u32 b = 0; b < in.nblk(); ++b)
    if (out.bsum[b] != off[b]) return fmt("bsum[%u] = %llu, serial scan %llu", b, out.bsum[b], off[b]);
  return "";
}

static void host_place(std::vector<u64>& table, u64 slots, u64 fp, u64 w) {
  u64 s = fp & (slots - 1);
  while (table[2 * s]) s = (s + 1) & (slots - 1);
  table[2 * s] = fp; table[2 * s + 1] = w;
}

static PipeIn make_pipe(u64 chunk, Rng& g) {
  PipeIn in;
  in.chunk_count = chunk; in.chunk_begin = (1ull << 33) + 4242; in.rank0 = 77777; in.nslot = 70; in.level = 5; in.smw = 2;
  in.slots = 1ull << 14;
  in.cand.assign(in.nslot * chunk, 0); in.smask.assign(in.smw * chunk, 0); in.table.assign(2 * in.slots, 0);
  in.cells.assign(in.nblk() * BS * in.nslot, 0xEEEEEEEEu); in.cell_count.assign(8 * in.nblk(), 0);
  const u64 mask = in.slots - 1;
  std::vector<u64> fresh(3 * chunk + 4), old(chunk / 2 + 2), later(chunk / 2 + 2), cluster(chunk < 20 ? 2 * chunk + 2 : 40);
  for (auto& f : fresh) f = g.fp();
  for (auto& f : cluster) f = (g.next() & ~mask) | (mask - 5);             // one home slot: the cluster wraps the table's end
  for (auto& f : old) { f = g.fp(); host_place(in.table, in.slots, f, ~((3ull << 40) | g.below(1ull << 30))); }   // an older level's
  const u64 beyond = (in.rank0 + chunk + 1000) * in.nslot;                 // this level's, from a producer behind this chunk
  for (auto& f : later) { f = g.fp(); host_place(in.table, in.slots, f, ~((in.level << 40) | (beyond + g.below(1000)))); }
  for (u64 st = 0; st < chunk; ++st) {
    const u32 b = (u32)(st / BS), w = (u32)(st % BS) / 64;
    if (chunk >= 128 && w == 1) continue;                                  // a wave without cells
    for (u64 sl = 0; sl < in.nslot; ++sl) {
      if (g.below(chunk == 1 ? 3 : 8)) continue;
      const u64 k = g.below(16);
      const std::vector<u64>& pool = k < 8 ? fresh : k < 11 ? old : k < 14 ? later : cluster;
      const u32 cell = (u32)(sl * chunk + st);
      in.cand[cell] = pool[g.below(pool.size())];
      in.smask[(sl / 64) * chunk + st] |= 1ull << (sl % 64);
      in.cells[b * BS * in.nslot + w * 64 * in.nslot + in.cell_count[8 * b + w]++] = cell;
    }
  }
  return in;
}

struct ScanOut { std::vector<unsigned long long> bsum; u64 total = 0; };
static ScanOut run_scan(const std::vector<unsigned long long>& v) {
  ssc::DevBuf<unsigned long long> bsum(v), ctr(std::vector<unsigned long long>(C_NCTR, 0));
  hipLaunchKernelGGL(memb_scan_blocks, dim3(1), dim3(BS), 0, 0, bsum.p, (u32)v.size(), ctr.p);
  ssc::launched("memb_scan_blocks");
  return {bsum.get(), ctr.get()[C_NEW]};
}
static ScanOut play_scan(const std::vector<unsigned long long>& v) {
  ScanOut o;
  for (auto c : v) { o.bsum.push_back(o.total); o.total += c; }
  return o;
}
static std::string check_scan(const std::vector<unsigned long long>& v, const ScanOut& out) {
  std::vector<unsigned long long> off;
  const u64 total = ssc::serial_scan(v, off);
  if (out.bsum.size() != off.size()) return "bsum size";
  for (size_t b = 0; b < off.size(); ++b)
    if (out.bsum[b] != off[b]) return fmt("bsum[%zu] = %llu, serial scan %llu", b, out.bsum[b], off[b]);
  if (out.total != total) return fmt("ctr[C_NEW] = %llu, total %llu", (unsigned long long)out.total, (unsigned long long)total);
  return "";
}

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    if (!std::strcmp(argv[i], "--host-only")) g_host_only = true;
    else { std::fprintf(stderr, "usage: memb_seen_set_check [--host-only]\n"); return 64; }
  }
  bool ok = true;
  Rng g(0x5EED0010);
  for (u64 chunk : {1ull, 255ull, 257ull, 1000ull}) {
    const PipeIn in = make_pipe(chunk, g);
    Report r;
    r.name = fmt("memb_pipeline_chunk_%llu", (unsigned long long)chunk);
    std::set<u64> fps;
    for (u32 c : cells_in_key_order(in)) { fps.insert(in.cand[c]); ++r.n; }
    r.distinct = fps.size();
    r.props["nslot"] = (long long)in.nslot;
    r.props["blocks"] = in.nblk();
    PipeOut out = g_host_only ? play_pipe(in) : run_pipe(in);
    r.props["wraps"] = out.table[2 * (in.slots - 1)] != 0 && out.table[0] != 0;
    const std::string m = check_pipe(in, out);
    r.fail(m);
    if (g_host_only && m.empty()) {
      auto chk = [&](const PipeOut& o) { return check_pipe(in, o); };
      ssc::try_perturb<PipeOut>(r, ssc::P_DROP, out, chk, [](PipeOut& o) { if (o.newrec.empty()) return false; o.newrec.erase(o.newrec.begin()); --o.c_new; return true; });
      ssc::try_perturb<PipeOut>(r, ssc::P_DUP, out, chk, [](PipeOut& o) { if (o.newrec.size() < 2) return false; o.newrec[1] = o.newrec[0]; return true; });
      ssc::try_perturb<PipeOut>(r, ssc::P_KEY_RAISED, out, chk, [&](PipeOut& o) { for (u64 s = 0; s < in.slots; ++s) if (o.table[2 * s]) { o.table[2 * s + 1] -= 1; return true; } return false; });
      ssc::try_perturb<PipeOut>(r, ssc::P_COUNT_TWICE, out, chk, [](PipeOut& o) { ++o.c_new; return true; });
      ssc::try_perturb<PipeOut>(r, ssc::P_SWAP, out, chk, [](PipeOut& o) { if (o.newrec.size() < 2) return false; std::swap(o.newrec[0], o.newrec[1]); return true; });
      ssc::try_perturb<PipeOut>(r, ssc::P_WOFF, out, chk, [](PipeOut& o) { ++o.woff.back(); return true; });
    }
    r.print();
    ok &= r.first.empty();
  }
  for (u32 nblocks : {1u, (u32)BS, (u32)SCAN_MAX_BLOCKS - 1, (u32)SCAN_MAX_BLOCKS}) {
    std::vector<unsigned long long> v(nblocks);
    for (auto& c : v) c = g.below(3) ? g.below(BS * 70 + 1) : 0;
    v.back() = BS * 70;
    Report r;
    r.name = fmt("memb_scan_blocks_%u", nblocks);
    r.n = nblocks;
    for (auto c : v) r.distinct += c;
    ScanOut out = g_host_only ? play_scan(v) : run_scan(v);
    const std::string m = check_scan(v, out);
    r.fail(m);
    if (g_host_only && m.empty()) {
      auto chk = [&](const ScanOut& o) { return check_scan(v, o); };
      ssc::try_perturb<ScanOut>(r, ssc::P_WOFF, out, chk, [](ScanOut& o) { ++o.bsum.back(); return true; });
      ssc::try_perturb<ScanOut>(r, ssc::P_COUNT_TWICE, out, chk, [](ScanOut& o) { ++o.total; return true; });
    }
    r.print();
    ok &= r.first.empty();
  }
  return ok ? 0 : 1;
}
