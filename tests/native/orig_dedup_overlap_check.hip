// TEST HARNESS ONLY (never part of the product).  The instantiation of orig_dedup_plain that runs beside a
// generate (OVERLAP_DEDUP_PER probes in flight per thread, an OVERLAP_LDS_FP_SLOTS-slot filter in the launch's
// dynamic LDS), launched once per case on a synthetic, seeded input and checked against the sequential model that
// orig_seen_set_check.hip uses for the stand-alone instantiation.  The backend translation unit is included as
// it stands, so the kernel is the product's own text.
//   orig_dedup_overlap_check [--host-only]   -> one JSON line per case (seen_set_check.h: Report)
// --host-only makes no HIP call: the outputs come from a sequential host routine that plays the kernel, go
// through the same check function, and are then perturbed to show that the check can fail.
// Every case: 3 workgroups, a 1024-record region (4 wave regions of 256), a 4096-slot seen-set.
#include "../../raft-tla_amd/csrc/orig_backend.hip"

#include "seen_set_check.h"

using namespace rmc;
using ssc::fmt;
using ssc::Report;
using ssc::Rng;

static bool g_host_only = false;
static const u64 JUNK = 0xEEEEEEEEEEEEEEEEull;   // prefill of what the kernel does not clear
constexpr int OVL_PER = OVERLAP_DEDUP_PER, OVL_SLOTS = OVERLAP_LDS_FP_SLOTS;
constexpr u64 REGION = 1024, TABLE_SLOTS = 4096;
constexpr u32 NBLK = 3;

// ====================================================================== record regions (generate's output)
struct RegIn {
  u64 gid0 = 0;
  std::vector<u64> rfp;
  std::vector<unsigned short> rkey;
  std::vector<u32> rcnt;
};
struct PRec { u64 fp; u32 lk; };
// block b's records in the order the kernel reads them (wave regions concatenated)
static std::vector<PRec> records_of(const RegIn& in, u32 b) {
  std::vector<PRec> v;
  const u64 wreg = REGION / 4;
  for (u32 w = 0; w < 4; ++w)
    for (u32 i = 0; i < in.rcnt[4 * b + w]; ++i) {
      const u64 at = b * REGION + w * wreg + i;
      v.push_back({in.rfp[at], in.rkey[at]});
    }
  return v;
}
// blocks[b]: the fingerprints of workgroup b, dealt to its waves by counts[b]; record i of wave w gets the
// local key of lane w * 64 + i % 64, instance i / 64
static RegIn make_regions(u64 gid0, const std::vector<std::vector<u64>>& blocks, const std::vector<std::vector<u32>>& counts) {
  RegIn in;
  in.gid0 = gid0;
  in.rfp.assign(NBLK * REGION, JUNK); in.rkey.assign(NBLK * REGION, 0xEEEE); in.rcnt.assign(4 * NBLK, 0);
  const u64 wreg = REGION / 4;
  if (blocks.size() != NBLK || counts.size() != NBLK) { std::printf("{\"error\": \"bad case: workgroups\"}\n"); std::exit(2); }
  for (u32 b = 0; b < NBLK; ++b) {
    size_t k = 0;
    for (u32 w = 0; w < 4; ++w) {
      const u32 c = counts[b][w];
      if (c > wreg || k + c > blocks[b].size()) { std::printf("{\"error\": \"bad case: wave count\"}\n"); std::exit(2); }
      in.rcnt[4 * b + w] = c;
      for (u32 i = 0; i < c; ++i, ++k) {
        in.rfp[b * REGION + w * wreg + i] = blocks[b][k];
        in.rkey[b * REGION + w * wreg + i] = (unsigned short)(((w * 64 + i % 64) << 8) | (i / 64));
      }
    }
    if (k != blocks[b].size()) { std::printf("{\"error\": \"bad case: wave counts do not add up\"}\n"); std::exit(2); }
  }
  return in;
}
static u64 key_of(const RegIn& in, u32 b, u32 lk) { return ~nkey_of(in.gid0, b, lk); }
static u64 with_lds_home(Rng& g, u32 home, u32 slots) { return (g.fp() & ~((u64)(slots - 1) << 20)) | ((u64)home << 20) | 1; }
static std::vector<u64> ordinary(Rng& g, size_t n) { std::vector<u64> v(n); for (auto& f : v) f = g.fp(); return v; }
static void host_place(std::vector<u64>& table, u64 fp) {
  u64 s = fp & (TABLE_SLOTS - 1);
  while (table[s]) s = (s + 1) & (TABLE_SLOTS - 1);
  table[s] = fp;
}

// ====================================================================== the launch, its model, its contract
struct PlainIn { RegIn reg; std::vector<u64> table; };
struct PlainOut { std::vector<u64> table, newpos; u64 chunk_new = 0, err = 0; };

static PlainOut run_plain(const PlainIn& in) {
  ssc::DevBuf<u64> rfp(in.reg.rfp), table(in.table), newpos(std::vector<u64>(NBLK * REGION + 1, JUNK));
  ssc::DevBuf<unsigned short> rkey(in.reg.rkey);
  ssc::DevBuf<u32> rcnt(in.reg.rcnt);
  ssc::DevBuf<unsigned long long> ctr(std::vector<unsigned long long>(K_NCTR, 0));
  DedupArgs a{};
  a.rfp = rfp.p; a.rkey = rkey.p; a.rcnt = rcnt.p; a.region = REGION; a.gid0 = in.reg.gid0; a.table = table.p;
  a.table_mask = TABLE_SLOTS - 1; a.newpos = newpos.p; a.ctr = ctr.p;
  hipLaunchKernelGGL((orig_dedup_plain<1, false, OVL_PER, OVL_SLOTS, true>), dim3(NBLK), dim3(BS), OVERLAP_FILTER_LDS, 0, a);
  ssc::launched("orig_dedup_plain (overlap)");
  PlainOut o;
  o.table = table.get(); o.newpos = newpos.get();
  o.chunk_new = ctr.get()[K_CHUNK_NEW]; o.err = ctr.get()[K_ERR];
  o.newpos.resize(o.chunk_new < o.newpos.size() ? o.chunk_new : o.newpos.size());
  return o;
}

// the kernel played sequentially: workgroup after workgroup, records in order, an exact per-workgroup filter
static PlainOut play_plain(const PlainIn& in) {
  PlainOut o;
  o.table = in.table;
  const u64 mask = TABLE_SLOTS - 1;
  for (u32 b = 0; b < NBLK; ++b) {
    std::set<u64> here, winners;
    for (auto& r : records_of(in.reg, b)) {
      if (!here.insert(r.fp).second) continue;
      u64 s = r.fp & mask;
      while (o.table[s] && o.table[s] != r.fp) s = (s + 1) & mask;
      if (o.table[s] == 0) { o.table[s] = r.fp; winners.insert(key_of(in.reg, b, r.lk)); }
    }
    for (u64 k : winners) o.newpos.push_back(k);
  }
  o.chunk_new = o.newpos.size();
  return o;
}

static std::string check_plain(const PlainIn& in, const PlainOut& out) {
  std::set<u64> before, absent, after;
  for (u64 f : in.table) if (f) before.insert(f);
  std::unordered_map<u64, u64> producer;   // key -> fp
  for (u32 b = 0; b < NBLK; ++b)
    for (auto& r : records_of(in.reg, b)) {
      if (!before.count(r.fp)) absent.insert(r.fp);
      producer[key_of(in.reg, b, r.lk)] = r.fp;
    }
  if (out.err) return fmt("ctr[K_ERR] = %llx", (unsigned long long)out.err);
  if (out.chunk_new != absent.size()) return fmt("ctr[K_CHUNK_NEW] = %llu, %zu fingerprints were absent", (unsigned long long)out.chunk_new, absent.size());
  if (out.newpos.size() != out.chunk_new) return "fewer records than ctr[K_CHUNK_NEW]";
  if (out.table.size() != in.table.size()) return "table size";
  for (u64 f : out.table) if (f && !after.insert(f).second) return fmt("fingerprint %016llx is stored twice", (unsigned long long)f);
  std::set<u64> all = before;
  all.insert(absent.begin(), absent.end());
  if (after != all) return fmt("the table holds %zu fingerprints, %zu expected", after.size(), all.size());
  std::set<u64> named, closed;
  u64 cur_blk = ~0ull, last = 0;
  for (size_t i = 0; i < out.newpos.size(); ++i) {
    const u64 rec = out.newpos[i];
    auto it = producer.find(rec);
    if (it == producer.end()) return fmt("newpos[%zu] = %llx is no producer of the input", i, (unsigned long long)rec);
    if (!absent.count(it->second)) return fmt("newpos[%zu] names %016llx, which the table already held", i, (unsigned long long)it->second);
    if (!named.insert(it->second).second) return fmt("fingerprint %016llx has two winners", (unsigned long long)it->second);
    const u64 blk = ((rec >> 8) - in.reg.gid0) / BS;
    if (blk != cur_blk) {
      if (!closed.insert(blk).second) return fmt("workgroup %llu's records are not contiguous", (unsigned long long)blk);
      cur_blk = blk;
    } else if (rec <= last) {
      return fmt("newpos[%zu] = %llx does not ascend within its workgroup", i, (unsigned long long)rec);
    }
    last = rec;
  }
  return "";
}

static Report plain_case(const std::string& name, const PlainIn& in) {
  Report r;
  r.name = name;
  std::set<u64> fps;
  u32 max_blk = 0, min_blk = ~0u;
  for (u32 b = 0; b < NBLK; ++b) {
    const std::vector<PRec> recs = records_of(in.reg, b);
    for (auto& x : recs) { fps.insert(x.fp); ++r.n; }
    max_blk = recs.size() > max_blk ? (u32)recs.size() : max_blk;
    min_blk = recs.size() < min_blk ? (u32)recs.size() : min_blk;
  }
  r.distinct = fps.size();
  u64 present = 0;
  for (u64 f : in.table) present += f != 0 && fps.count(f);
  r.props["per"] = OVL_PER;
  r.props["lds_slots"] = OVL_SLOTS;
  r.props["rounds_max"] = (max_blk + OVL_PER * BS - 1) / (OVL_PER * BS);   // trips of the kernel's record loop
  r.props["records_max"] = max_blk;
  r.props["records_min"] = min_blk;
  r.props["present"] = (long long)present;
  r.props["max_per_lds_home"] = ssc::WindowModel(fps, OVL_SLOTS, LDS_WIN).max_per_home();
  PlainOut out = g_host_only ? play_plain(in) : run_plain(in);
  r.props["wraps"] = out.table[TABLE_SLOTS - 1] != 0 && out.table[0] != 0;
  const std::string m = check_plain(in, out);
  r.fail(m);
  if (g_host_only && m.empty()) {
    auto chk = [&](const PlainOut& o) { return check_plain(in, o); };
    const u64 gid0 = in.reg.gid0;
    ssc::try_perturb<PlainOut>(r, ssc::P_DROP, out, chk, [](PlainOut& o) {
      if (o.newpos.empty()) return false;
      o.newpos.pop_back(); --o.chunk_new;
      return true; });
    ssc::try_perturb<PlainOut>(r, ssc::P_DUP, out, chk, [](PlainOut& o) {
      if (o.newpos.empty()) return false;
      o.newpos.insert(o.newpos.begin(), o.newpos[0]); ++o.chunk_new;
      return true; });
    ssc::try_perturb<PlainOut>(r, ssc::P_COUNT_TWICE, out, chk, [](PlainOut& o) { ++o.chunk_new; return true; });
    ssc::try_perturb<PlainOut>(r, ssc::P_SWAP, out, chk, [gid0](PlainOut& o) {   // two winners of one workgroup
      for (size_t i = 0; i + 1 < o.newpos.size(); ++i)
        if (((o.newpos[i] >> 8) - gid0) / BS == ((o.newpos[i + 1] >> 8) - gid0) / BS) { std::swap(o.newpos[i], o.newpos[i + 1]); return true; }
      return false; });
  }
  return r;
}

// ====================================================================== cases
// n records drawn from a pool (so that some repeat inside the workgroup)
static std::vector<u64> draw(Rng& g, const std::vector<u64>& pool, u32 n) {
  std::vector<u64> v;
  for (u32 i = 0; i < n; ++i) v.push_back(pool[i < pool.size() ? i : g.below(pool.size())]);
  g.shuffle(v);
  return v;
}

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    if (!std::strcmp(argv[i], "--host-only")) g_host_only = true;
    else { std::fprintf(stderr, "usage: orig_dedup_overlap_check [--host-only]\n"); return 64; }
  }
  static_assert(OVL_PER * BS == 512, "the record counts below sit on the PER * BS boundary");
  static_assert(OVL_SLOTS == 4096, "the window case's home is the last slots of a 4096-slot filter");
  std::vector<Report> all;
  auto emit = [&](const Report& r) { r.print(); all.push_back(r); };   // a line per case as soon as it is done
  Rng g(0x5EED0F01);
  const u64 gid0 = (1ull << 34) + 4242;

  // record counts on the PER * BS boundary, spread unevenly over the four wave regions.  Workgroups 0 and 2
  // hold n records each (two different splits), workgroup 1 a hundred, all in wave 2
  struct Split { u32 n; std::vector<u32> a, b; };
  const std::vector<Split> splits = {
      {0, {0, 0, 0, 0}, {0, 0, 0, 0}},
      {1, {0, 0, 1, 0}, {0, 0, 0, 1}},
      {511, {256, 43, 212, 0}, {1, 254, 0, 256}},
      {512, {256, 0, 256, 0}, {100, 156, 256, 0}},
      {513, {256, 1, 256, 0}, {129, 128, 0, 256}},
  };
  for (const Split& sp : splits) {
    PlainIn in;
    in.table.assign(TABLE_SLOTS, 0);
    const std::vector<u64> pool = ordinary(g, sp.n ? (sp.n * 3 + 3) / 4 : 1), mid = ordinary(g, 60);
    std::vector<u64> b1 = draw(g, mid, 100);
    for (size_t i = 0; i < pool.size() && i < 20; ++i) b1[i] = pool[i];      // across workgroups
    for (size_t i = 0; i < pool.size(); i += 4) host_place(in.table, pool[i]);   // a quarter is already in the table
    for (size_t i = 0; i < mid.size(); i += 3) host_place(in.table, mid[i]);
    in.reg = make_regions(gid0, {draw(g, pool, sp.n), b1, draw(g, pool, sp.n)}, {sp.a, {0, 0, 100, 0}, sp.b});
    emit(plain_case(fmt("overlap_records_%u", sp.n), in));
  }
  {   // 24 fingerprints of one LDS home, the 8-slot window wrapping the filter's end: twice in workgroup 2, once
      // in workgroup 0, a third already in the table; a full window passes records through to the seen-set
    PlainIn in;
    in.table.assign(TABLE_SLOTS, 0);
    const std::vector<u64> A = ordinary(g, 120);
    std::set<u64> one;
    while (one.size() < 24) one.insert(with_lds_home(g, OVL_SLOTS - 4, OVL_SLOTS));
    std::vector<u64> b0(A.begin(), A.begin() + 80), b1(A.begin() + 40, A.end()), b2(A.begin(), A.begin() + 20);
    for (u64 f : one) { b2.push_back(f); b2.push_back(f); b0.push_back(f); }
    g.shuffle(b0); g.shuffle(b1); g.shuffle(b2);
    { int i = 0; for (u64 f : one) if (i++ % 3 == 0) host_place(in.table, f); }
    for (int i = 60; i < 100; ++i) host_place(in.table, A[i]);
    in.reg = make_regions(gid0, {b0, b1, b2}, {{40, 0, (u32)b0.size() - 60, 20}, {20, 20, 20, 20}, {0, (u32)b2.size(), 0, 0}});
    Report r = plain_case("overlap_lds_window_wraps", in);
    r.props["home"] = OVL_SLOTS - 4;
    emit(r);
  }
  {   // 200 fingerprints repeated inside a workgroup and across workgroups, 100 of them already in the table
    PlainIn in;
    in.table.assign(TABLE_SLOTS, 0);
    const std::vector<u64> A = ordinary(g, 200);
    std::vector<u64> b0(A.begin(), A.begin() + 150), b1(A.begin() + 50, A.end()), b2(A.begin() + 100, A.end());
    for (int i = 0; i < 150; ++i) b0.push_back(A[g.below(150)]);             // repeated inside one workgroup
    for (int i = 0; i < 100; ++i) b2.push_back(A[100 + g.below(100)]);
    for (int i = 0; i < 150; ++i) b1.push_back(A[50 + i]);                   // every fingerprint of workgroup 1 twice
    g.shuffle(b0); g.shuffle(b1); g.shuffle(b2);
    for (int i = 50; i < 150; ++i) host_place(in.table, A[i]);
    in.reg = make_regions(gid0, {b0, b1, b2}, {{150, 0, 100, 50}, {75, 75, 75, 75}, {0, 0, 200, 0}});
    emit(plain_case("overlap_duplicates", in));
  }
  {   // one seen-set cluster across the table's end: 60 fingerprints of home 4090, a third of them placed before
    PlainIn in;
    in.table.assign(TABLE_SLOTS, 0);
    std::set<u64> fps;
    while (fps.size() < 60) fps.insert((g.next() & ~(TABLE_SLOTS - 1)) | (TABLE_SLOTS - 6));
    std::vector<u64> v(fps.begin(), fps.end());
    g.shuffle(v);
    for (int i = 0; i < 20; ++i) host_place(in.table, v[i]);
    std::vector<u64> b0(v.begin(), v.begin() + 40), b1(v.begin() + 10, v.end()), b2(v.begin() + 30, v.end());
    for (int i = 30; i < 60; ++i) b2.push_back(v[i]);
    g.shuffle(b0); g.shuffle(b1); g.shuffle(b2);
    in.reg = make_regions(gid0, {b0, b1, b2}, {{0, 0, 40, 0}, {13, 12, 0, 25}, {30, 30, 0, 0}});
    Report r = plain_case("overlap_table_cluster_wraps", in);
    r.props["home"] = (long long)(TABLE_SLOTS - 6);
    emit(r);
  }
  bool ok = true;
  for (auto& r : all) ok &= r.first.empty();
  return ok ? 0 : 1;
}
