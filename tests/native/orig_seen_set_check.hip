// TEST HARNESS ONLY (never part of the product).  raft_original's seen-set and dedup kernels, each run
// once on a synthetic, seeded, adversarial input and checked against a plain sequential model:
// orig_probe / orig_dedup_sh (probe_batch), orig_merge (lds_merge, WaveRegions), orig_dedup_plain
// (lds_first), orig_mark + orig_count + orig_scan, orig_migrate<1|2>, orig_route_blk.  The backend
// translation unit is included as it stands, so the kernels are the product's own text.
//   orig_seen_set_check [--host-only]   -> one JSON line per case (seen_set_check.h: Report)
// --host-only makes no HIP call: the outputs come from sequential host routines that play the kernels,
// go through the same check functions, and are then perturbed to show that the checks can fail.
// Which lane wins a race is not fixed, so every contract is on sets, counts and minima; positions are
// compared only where the kernel promises an order.
#include "../../raft-tla_amd/csrc/orig_backend.hip"

#include "seen_set_check.h"

using namespace rmc;
using ssc::fmt;
using ssc::Report;
using ssc::Rng;

static bool g_host_only = false;
// a case's line goes out as soon as the case is done: what ran before a HIP failure stays on record
static void emit(std::vector<Report>& all, const Report& r) { r.print(); all.push_back(r); }
static const u64 KEY_MAX = (((1ull << 40) - 1) << 8) | 255ull;   // gid just below 2^40, instance 255
static const u64 JUNK = 0xEEEEEEEEEEEEEEEEull;                    // prefill of output regions the kernels do not clear

// ====================================================================== orig_probe / orig_dedup_sh
struct Rec { u64 fp, w; };   // w: ~key (orig_probe) or the record's slot word (orig_dedup_sh)
struct ProbeIn {
  bool sh = false;                       // orig_dedup_sh (8-B entries) instead of orig_probe (16-B {fp, ~key})
  u64 slots = 0;
  std::vector<u64> table;                // before the launch
  std::vector<std::vector<Rec>> blk;     // orig_probe: one region per workgroup; orig_dedup_sh: concatenated
  bool expect_full = false, expect_identical = false;
};
struct ProbeOut {
  std::vector<u64> table;
  u64 ins = 0, err = 0;
  std::vector<u64> rep;                  // newpos (orig_probe) / reply slot words (orig_dedup_sh): ins of them
};
constexpr u64 PROBE_REGION = 1024;

static ProbeOut run_probe(const ProbeIn& in) {
  ProbeOut o;
  u64 total = 0;
  for (auto& b : in.blk) total += b.size();
  ssc::DevBuf<u64> table(in.table), rep(std::vector<u64>(total + 1, JUNK));
  ssc::DevBuf<unsigned long long> ctr(std::vector<unsigned long long>(K_NCTR, 0)), counter(std::vector<unsigned long long>(1, 0));
  if (!in.sh) {
    const u32 nblk = (u32)in.blk.size();
    std::vector<ulonglong2> urec(nblk * PROBE_REGION, make_ulonglong2(JUNK, JUNK));
    std::vector<u32> ucnt(nblk);
    for (u32 b = 0; b < nblk; ++b) {
      if (in.blk[b].size() > PROBE_REGION) { std::printf("{\"error\": \"probe region too small\"}\n"); std::exit(2); }
      ucnt[b] = (u32)in.blk[b].size();
      for (size_t i = 0; i < in.blk[b].size(); ++i) urec[b * PROBE_REGION + i] = make_ulonglong2(in.blk[b][i].fp, in.blk[b][i].w);
    }
    ssc::DevBuf<ulonglong2> durec(urec);
    ssc::DevBuf<u32> ducnt(ucnt);
    DedupArgs a{};
    a.region = PROBE_REGION; a.urec = durec.p; a.ucnt = ducnt.p; a.table = table.p; a.table_mask = in.slots - 1;
    a.newpos = rep.p; a.ctr = ctr.p; a.prof = 0;
    hipLaunchKernelGGL((orig_probe<false>), dim3(nblk), dim3(BS), 0, 0, a);
    ssc::launched("orig_probe");
    o.ins = ctr.get()[K_INS];
  } else {
    std::vector<u64> recv;
    for (auto& b : in.blk) for (auto& r : b) { recv.push_back(r.fp); recv.push_back(r.w); }
    ssc::DevBuf<u64> drecv(recv);
    DedupShArgs a{};
    a.recv = drecv.p; a.n = total; a.table = table.p; a.table_mask = in.slots - 1; a.reply = rep.p; a.counter = counter.p; a.ctr = ctr.p;
    hipLaunchKernelGGL(orig_dedup_sh, dim3((unsigned)((total + BS * DEDUP_PER - 1) / (BS * DEDUP_PER))), dim3(BS), 0, 0, a);
    ssc::launched("orig_dedup_sh");
    o.ins = counter.get()[0];
  }
  o.err = ctr.get()[K_ERR];
  o.table = table.get();
  o.rep = rep.get();
  o.rep.resize(o.ins < total + 1 ? o.ins : total + 1);
  return o;
}

// the kernel played sequentially: records in order, linear probing from the home slot
static ProbeOut play_probe(const ProbeIn& in) {
  ProbeOut o;
  o.table = in.table;
  const u64 st = in.sh ? 1 : 2, mask = in.slots - 1;
  for (auto& b : in.blk)
    for (auto& r : b) {
      u64 s = r.fp & mask, k = 0;
      for (; k < in.slots; ++k, s = (s + 1) & mask)
        if (o.table[st * s] == r.fp || o.table[st * s] == 0) break;
      if (k == in.slots) { o.err |= OE_TABLE_FULL; continue; }
      if (o.table[st * s] == 0) { o.table[st * s] = r.fp; ++o.ins; o.rep.push_back(in.sh ? r.w : s); }
      if (!in.sh && o.table[2 * s + 1] < r.w) o.table[2 * s + 1] = r.w;
    }
  return o;
}

static std::string check_probe(const ProbeIn& in, const ProbeOut& out) {
  const u64 st = in.sh ? 1 : 2;
  if (out.table.size() != in.table.size()) return "table size";
  if (in.expect_full) {
    if (!(out.err & OE_TABLE_FULL)) return fmt("ctr[K_ERR] = %llx, OE_TABLE_FULL expected", (unsigned long long)out.err);
    if (out.table != in.table) return "the stored entries changed although the table was full";
    if (out.ins) return fmt("%llu insertions into a full table", (unsigned long long)out.ins);
    return "";
  }
  std::unordered_map<u64, u64> want;   // fp -> ~(minimum key) = maximum complement
  std::set<u64> before, absent;
  for (u64 s = 0; s < in.slots; ++s)
    if (u64 f = in.table[st * s]) { before.insert(f); want[f] = in.sh ? 0 : in.table[2 * s + 1]; }
  std::unordered_map<u64, u64> word_fp;   // orig_dedup_sh: slot word -> its record's fp
  for (auto& b : in.blk)
    for (auto& r : b) {
      if (!before.count(r.fp)) absent.insert(r.fp);
      auto it = want.find(r.fp);
      const u64 w = in.sh ? 0 : r.w;
      if (it == want.end()) want[r.fp] = w; else if (it->second < w) it->second = w;
      word_fp[r.w] = r.fp;
    }
  if (out.err) return fmt("ctr[K_ERR] = %llx", (unsigned long long)out.err);
  if (out.ins != absent.size()) return fmt("%llu insertions counted, %zu fingerprints were absent", (unsigned long long)out.ins, absent.size());
  std::set<u64> stored;
  for (u64 s = 0; s < in.slots; ++s) {
    const u64 f = out.table[st * s];
    if (!f) continue;
    auto it = want.find(f);
    if (it == want.end()) return fmt("slot %llu holds %016llx, which nobody gave", (unsigned long long)s, (unsigned long long)f);
    if (!stored.insert(f).second) return fmt("fingerprint %016llx is stored twice (second at slot %llu)", (unsigned long long)f, (unsigned long long)s);
    if (!in.sh && out.table[2 * s + 1] != it->second)
      return fmt("fingerprint %016llx: key %llx, minimum given %llx", (unsigned long long)f, (unsigned long long)~out.table[2 * s + 1], (unsigned long long)~it->second);
  }
  if (stored.size() != want.size()) return fmt("%zu fingerprints stored, %zu expected: a fingerprint was lost", stored.size(), want.size());
  if (in.expect_identical && out.table != in.table) return "the table changed on a launch that had nothing to add";
  if (out.rep.size() != out.ins) return "fewer positions than insertions";
  std::set<u64> named, seen_rep;
  for (u64 v : out.rep) {
    if (!seen_rep.insert(v).second) return fmt("position/slot word %llx reported twice", (unsigned long long)v);
    u64 f;
    if (in.sh) {
      auto it = word_fp.find(v);
      if (it == word_fp.end()) return fmt("reply %llx is no record's slot word", (unsigned long long)v);
      f = it->second;
    } else {
      if (v >= in.slots) return fmt("newpos %llx is outside the table", (unsigned long long)v);
      f = out.table[2 * v];
    }
    if (!absent.count(f)) return fmt("reported entry holds %016llx, which was not inserted by this launch", (unsigned long long)f);
    if (!named.insert(f).second) return fmt("fingerprint %016llx reported as inserted twice", (unsigned long long)f);
  }
  return "";
}

// linear-probing placement of an entry while building an input table
static void host_place(std::vector<u64>& table, u64 slots, u64 st, u64 fp, u64 w) {
  u64 s = fp & (slots - 1);
  while (table[st * s]) s = (s + 1) & (slots - 1);
  table[st * s] = fp;
  if (st == 2) table[2 * s + 1] = w;
}

static u64 rand_key(Rng& g) { return (g.below(1ull << 40) << 8) | g.below(256); }

// steps[k].table (k > 0) is what step k - 1 left
static Report probe_case(const std::string& name, std::vector<ProbeIn> steps) {
  Report r;
  r.name = name;
  std::set<u64> fps;
  for (auto& b : steps[0].blk) { for (auto& x : b) fps.insert(x.fp); r.n += b.size(); }
  r.distinct = fps.size();
  r.props["slots"] = (long long)steps[0].slots;
  ProbeOut prev;
  for (size_t k = 0; k < steps.size(); ++k) {
    if (k) steps[k].table = prev.table;
    ProbeOut out = g_host_only ? play_probe(steps[k]) : run_probe(steps[k]);
    const std::string m = check_probe(steps[k], out);
    if (!m.empty()) r.fail(fmt("launch %zu: ", k + 1) + m);
    if (k == 0) {
      const u64 st = steps[0].sh ? 1 : 2;
      r.props["wraps"] = out.table[st * (steps[0].slots - 1)] != 0 && out.table[0] != 0;
      if (g_host_only && m.empty()) {
        const ProbeIn& in = steps[0];
        auto chk = [&](const ProbeOut& o) { return check_probe(in, o); };
        ssc::try_perturb<ProbeOut>(r, ssc::P_DROP, out, chk, [&](ProbeOut& o) {
          for (u64 s = 0; s < in.slots; ++s) if (o.table[st * s]) { o.table[st * s] = 0; if (st == 2) o.table[2 * s + 1] = 0; return true; }
          return false; });
        ssc::try_perturb<ProbeOut>(r, ssc::P_DUP, out, chk, [&](ProbeOut& o) {
          u64 from = in.slots, to = in.slots;
          for (u64 s = 0; s < in.slots; ++s) { if (o.table[st * s]) from = s; else to = s; }
          if (from == in.slots || to == in.slots) return false;
          for (u64 q = 0; q < st; ++q) o.table[st * to + q] = o.table[st * from + q];
          return true; });
        if (!in.sh)
          ssc::try_perturb<ProbeOut>(r, ssc::P_KEY_RAISED, out, chk, [&](ProbeOut& o) {
            for (u64 s = 0; s < in.slots; ++s) if (o.table[2 * s] && o.table[2 * s + 1]) { o.table[2 * s + 1] -= 1; return true; }
            return false; });
        ssc::try_perturb<ProbeOut>(r, ssc::P_COUNT_TWICE, out, chk, [&](ProbeOut& o) { o.ins += 1; return true; });
      }
    }
    prev = out;
  }
  return r;
}

static ProbeIn probe_empty(bool sh, u64 slots) {
  ProbeIn p;
  p.sh = sh; p.slots = slots; p.table.assign((sh ? 1 : 2) * slots, 0);
  return p;
}
// records dealt round-robin to nblk workgroups
static void deal(ProbeIn& p, const std::vector<Rec>& recs, u32 nblk) {
  p.blk.assign(nblk, {});
  for (size_t i = 0; i < recs.size(); ++i) p.blk[i % nblk].push_back(recs[i]);
}

static void probe_cases(bool sh, std::vector<Report>& all) {
  const std::string pre = sh ? "dedup_sh_" : "probe_";
  const u64 slots = 1024, mask = slots - 1;
  Rng g(sh ? 0x5EED0001 : 0x5EED0002);
  u64 word = 0;   // orig_dedup_sh slot words: unique per record
  auto w_of = [&](u64 key) -> u64 {
    if (!sh) return ~key;
    ++word;
    return (word << 8) | (word % 7);
  };
  // one home slot, wrapping: n distinct fingerprints, two producers each with different keys
  for (u32 n : {8u, 64u, 600u}) {
    ProbeIn p = probe_empty(sh, slots);
    std::set<u64> fps;
    while (fps.size() < n) fps.insert((g.next() & ~mask) | (mask - 3));
    std::vector<Rec> recs;
    for (u64 f : fps) { recs.push_back({f, w_of(rand_key(g))}); recs.push_back({f, w_of(rand_key(g))}); }
    g.shuffle(recs);
    deal(p, recs, n > 256 ? 3 : 1);
    Report r = probe_case(pre + fmt("one_home_%u", n), {p});
    r.props["home"] = (long long)(mask - 3);
    emit(all, r);
  }
  {   // one fingerprint, 4096 producers in 4 workgroups, the minimum key in the last one
    ProbeIn p = probe_empty(sh, slots);
    const u64 f = g.fp();
    std::vector<u64> keys(4096);
    for (u64 i = 0; i < 4096; ++i) keys[i] = ((i + 1) << 8) | 5;
    g.shuffle(keys);
    size_t mi = 0;
    for (size_t i = 0; i < keys.size(); ++i) if (keys[i] < keys[mi]) mi = i;
    std::swap(keys[mi], keys[3 * 1024 + 77]);
    p.blk.assign(4, {});
    for (size_t i = 0; i < keys.size(); ++i) p.blk[i / 1024].push_back({f, w_of(keys[i])});
    ProbeIn again = p, lower = p;
    again.expect_identical = true;
    for (auto& b : lower.blk) for (auto& x : b) x.w = sh ? x.w : x.w + 1;   // ~(key - 1)
    std::vector<ProbeIn> steps = {p, again};
    if (!sh) steps.push_back(lower);
    Report r = probe_case(pre + "one_fp_many", steps);
    r.props["min_key_block"] = 3;
    emit(all, r);
  }
  {   // extreme fingerprints and keys
    ProbeIn p = probe_empty(sh, slots);
    const u64 x = g.fp() | 1;
    std::vector<Rec> recs = {{1, w_of(KEY_MAX)}, {1, w_of(0)}, {~0ull, w_of(0)}, {1ull << 63, w_of(KEY_MAX)}, {mask + 1, w_of(KEY_MAX)},
                             {mask + 1, w_of(0)}, {x, w_of(KEY_MAX)}, {x ^ (1ull << 40), w_of(0)}, {x, w_of(KEY_MAX - 1)}, {~0ull, w_of(KEY_MAX)}};
    deal(p, recs, 1);
    emit(all, probe_case(pre + "extremes", {p}));
  }
  {   // exact fill, then one more
    ProbeIn p = probe_empty(sh, slots);
    std::set<u64> fps;
    while (fps.size() < slots) fps.insert(g.fp());
    std::vector<Rec> recs;
    for (u64 f : fps) recs.push_back({f, w_of(rand_key(g))});
    g.shuffle(recs);
    deal(p, recs, 4);
    ProbeIn more = probe_empty(sh, slots);
    u64 extra;
    do extra = g.fp(); while (fps.count(extra));
    deal(more, std::vector<Rec>{Rec{extra, w_of(rand_key(g))}}, 1);
    more.expect_full = true;
    emit(all, probe_case(pre + "exact_fill", {p, more}));
  }
  {   // pre-populated: half of the input present, half of those with the smaller key
    ProbeIn p = probe_empty(sh, slots);
    std::set<u64> fps;
    while (fps.size() < 512) fps.insert(g.fp());
    std::vector<Rec> recs;
    u32 i = 0;
    for (u64 f : fps) {
      const u64 key = rand_key(g) | 0x100;   // (room for key - 1)
      recs.push_back({f, w_of(key)});
      if (i % 2 == 0) host_place(p.table, slots, sh ? 1 : 2, f, ~((i % 4 == 0) ? key - 1 : key + 1));
      ++i;
    }
    g.shuffle(recs);
    deal(p, recs, 2);
    Report r = probe_case(pre + "prepopulated", {p});
    r.props["present"] = 256;
    emit(all, r);
  }
}

// ====================================================================== record regions (generate's output)
struct RegIn {
  u64 region = 0, gid0 = 0;
  u32 nblk = 0;
  std::vector<u64> rfp;
  std::vector<unsigned short> rkey;
  std::vector<u32> rcnt;
};
struct PRec { u64 fp; u32 lk; };
// block b's records in the order the kernels read them (wave regions concatenated)
static std::vector<PRec> records_of(const RegIn& in, u32 b) {
  std::vector<PRec> v;
  const u64 wreg = in.region / 4;
  for (u32 w = 0; w < 4; ++w)
    for (u32 i = 0; i < in.rcnt[4 * b + w]; ++i) {
      const u64 at = b * in.region + w * wreg + i;
      v.push_back({in.rfp[at], in.rkey[at]});
    }
  return v;
}
// blocks[b]: the fingerprints of workgroup b, dealt to its waves by counts[b]; record i of wave w gets the
// local key of lane w * 64 + i % 64, instance i / 64
static RegIn make_regions(u64 region, u64 gid0, const std::vector<std::vector<u64>>& blocks, const std::vector<std::vector<u32>>& counts) {
  RegIn in;
  in.region = region; in.gid0 = gid0; in.nblk = (u32)blocks.size();
  in.rfp.assign(in.nblk * region, JUNK); in.rkey.assign(in.nblk * region, 0xEEEE); in.rcnt.assign(4 * in.nblk, 0);
  const u64 wreg = region / 4;
  for (u32 b = 0; b < in.nblk; ++b) {
    size_t k = 0;
    for (u32 w = 0; w < 4; ++w) {
      const u32 c = counts[b][w];
      if (c > wreg || k + c > blocks[b].size()) { std::printf("{\"error\": \"bad case: wave count\"}\n"); std::exit(2); }
      in.rcnt[4 * b + w] = c;
      for (u32 i = 0; i < c; ++i, ++k) {
        in.rfp[b * region + w * wreg + i] = blocks[b][k];
        in.rkey[b * region + w * wreg + i] = (unsigned short)(((w * 64 + i % 64) << 8) | (i / 64));
      }
    }
    if (k != blocks[b].size()) { std::printf("{\"error\": \"bad case: wave counts do not add up\"}\n"); std::exit(2); }
  }
  return in;
}
static u64 key_of(const RegIn& in, u32 b, u32 lk) { return ~nkey_of(in.gid0, b, lk); }
static u64 with_lds_home(Rng& g, u32 home, u32 slots) { return (g.fp() & ~((u64)(slots - 1) << 20)) | ((u64)home << 20) | 1; }
static std::vector<u64> ordinary(Rng& g, size_t n) { std::vector<u64> v(n); for (auto& f : v) f = g.fp(); return v; }

// ====================================================================== orig_merge
struct MergeOut { std::vector<ulonglong2> urec; std::vector<u32> ucnt; };

static MergeOut run_merge(const RegIn& in) {
  ssc::DevBuf<u64> rfp(in.rfp);
  ssc::DevBuf<unsigned short> rkey(in.rkey);
  ssc::DevBuf<u32> rcnt(in.rcnt), ucnt(std::vector<u32>(in.nblk, 0xEEEEEEEEu));
  ssc::DevBuf<ulonglong2> urec(std::vector<ulonglong2>(in.nblk * in.region, make_ulonglong2(JUNK, JUNK)));
  DedupArgs a{};
  a.rfp = rfp.p; a.rkey = rkey.p; a.rcnt = rcnt.p; a.region = in.region; a.gid0 = in.gid0; a.urec = urec.p; a.ucnt = ucnt.p;
  hipLaunchKernelGGL(orig_merge, dim3(in.nblk), dim3(BS), 0, 0, a);
  ssc::launched("orig_merge");
  return {urec.get(), ucnt.get()};
}

static MergeOut play_merge(const RegIn& in) {
  MergeOut o;
  o.urec.assign(in.nblk * in.region, make_ulonglong2(JUNK, JUNK));
  o.ucnt.assign(in.nblk, 0);
  for (u32 b = 0; b < in.nblk; ++b) {
    std::vector<u64> lfp(LDS_FP_SLOTS, 0);
    std::vector<u32> lkey(LDS_FP_SLOTS, ~0u);
    std::vector<ulonglong2> ovf;
    for (auto& r : records_of(in, b)) {
      u32 h = (u32)(r.fp >> 20) & (LDS_FP_SLOTS - 1);
      int p = 0;
      for (; p < 8; ++p, h = (h + 1) & (LDS_FP_SLOTS - 1)) {
        if (lfp[h] == 0) lfp[h] = r.fp;
        if (lfp[h] == r.fp) { if (r.lk < lkey[h]) lkey[h] = r.lk; break; }
      }
      if (p == 8) ovf.push_back(make_ulonglong2(r.fp, nkey_of(in.gid0, b, r.lk)));
    }
    ulonglong2* out = o.urec.data() + b * in.region;
    u32 c = 0;
    for (int s = 0; s < LDS_FP_SLOTS; ++s) if (lfp[s]) out[c++] = make_ulonglong2(lfp[s], nkey_of(in.gid0, b, lkey[s]));
    for (auto& x : ovf) out[c++] = x;
    o.ucnt[b] = c;
  }
  return o;
}

static std::string check_merge(const RegIn& in, const MergeOut& out) {
  for (u32 b = 0; b < in.nblk; ++b) {
    const std::vector<PRec> recs = records_of(in, b);
    std::unordered_map<u64, u64> want;   // fp -> minimum key
    std::set<u64> fps;
    for (auto& r : recs) {
      const u64 k = key_of(in, b, r.lk);
      auto it = want.find(r.fp);
      if (it == want.end()) want[r.fp] = k; else if (k < it->second) it->second = k;
      fps.insert(r.fp);
    }
    const ssc::WindowModel win(fps, LDS_FP_SLOTS, 8);
    const u32 c = out.ucnt[b];
    if (c > recs.size()) return fmt("workgroup %u: ucnt %u > n %zu", b, c, recs.size());
    std::unordered_map<u64, u64> got;
    std::unordered_map<u64, u32> times;
    for (u32 i = 0; i < c; ++i) {
      const ulonglong2 x = out.urec[b * in.region + i];
      if (!want.count(x.x)) return fmt("workgroup %u: urec[%u] holds %016llx, which is no input fingerprint", b, i, (unsigned long long)x.x);
      const u64 k = ~x.y;
      auto it = got.find(x.x);
      if (it == got.end()) got[x.x] = k; else if (k < it->second) it->second = k;
      if (++times[x.x] > 1 && !win.may_be_full(x.x))
        return fmt("workgroup %u: fingerprint %016llx appears %u times although its window cannot have been full", b, (unsigned long long)x.x, times[x.x]);
    }
    for (auto& w : want) {
      auto it = got.find(w.first);
      if (it == got.end()) return fmt("workgroup %u: fingerprint %016llx is lost (%zu of %zu distinct survive)", b, (unsigned long long)w.first, got.size(), want.size());
      if (it->second != w.second) return fmt("workgroup %u: fingerprint %016llx: minimum key out %llx, in %llx", b, (unsigned long long)w.first, (unsigned long long)it->second, (unsigned long long)w.second);
    }
  }
  return "";
}

static Report merge_case(const std::string& name, const RegIn& in, u32 focus) {
  Report r;
  r.name = name;
  const std::vector<PRec> recs = records_of(in, focus);
  std::set<u64> fps;
  for (auto& x : recs) fps.insert(x.fp);
  r.n = recs.size(); r.distinct = fps.size();
  const ssc::WindowModel win(fps, LDS_FP_SLOTS, 8);
  r.props["region"] = (long long)in.region;
  r.props["max_per_lds_home"] = win.max_per_home();
  if (win.per_home.size() == 1) {   // one home: the window takes 8 fingerprints, every other record overflows
    // the number of overflow records does not depend on which 8 win when every fingerprint is given equally often
    const u64 per = r.distinct ? r.n / r.distinct : 0;
    const u64 merged = (r.distinct < 8 ? r.distinct : 8) * per;
    r.props["total"] = (long long)(r.distinct < 8 ? r.distinct : 8);
    r.props["nov"] = (long long)(r.n - merged);
  }
  MergeOut out = g_host_only ? play_merge(in) : run_merge(in);
  r.props["ucnt"] = out.ucnt[focus];
  const std::string m = check_merge(in, out);
  r.fail(m);
  if (g_host_only && m.empty()) {
    auto chk = [&](const MergeOut& o) { return check_merge(in, o); };
    ssc::try_perturb<MergeOut>(r, ssc::P_DROP, out, chk, [&](MergeOut& o) {
      u32& c = o.ucnt[focus];
      if (!c) return false;
      o.urec[focus * in.region] = o.urec[focus * in.region + c - 1];   // record 0 (a slot of the set) leaves
      --c;
      return true; });
    ssc::try_perturb<MergeOut>(r, ssc::P_DUP, out, chk, [&](MergeOut& o) {
      u32& c = o.ucnt[focus];
      if (!c || c >= in.region) return false;
      u32 pick = 0;
      for (u32 i = 0; i < c; ++i) if (!win.may_be_full(o.urec[focus * in.region + i].x)) { pick = i; break; }
      if (win.may_be_full(o.urec[focus * in.region + pick].x) && c < r.n) return false;
      o.urec[focus * in.region + c] = o.urec[focus * in.region + pick];
      ++c;
      return true; });
    ssc::try_perturb<MergeOut>(r, ssc::P_KEY_RAISED, out, chk, [&](MergeOut& o) {
      if (!o.ucnt[focus]) return false;
      o.urec[focus * in.region].y -= 1;
      return true; });
  }
  return r;
}

static void merge_cases(std::vector<Report>& all) {
  Rng g(0x5EED0003);
  const u64 gid0 = (1ull << 33) + 12345;
  const std::vector<u64> plain = ordinary(g, 100);
  const std::vector<u32> plain_cnt = {7, 0, 64, 29};
  {   // 64 fingerprints of one LDS home, three producers each, among ordinary records
    std::vector<u64> v = ordinary(g, 300);
    std::set<u64> one;
    while (one.size() < 64) one.insert(with_lds_home(g, 2045, LDS_FP_SLOTS));   // the window wraps the set's end
    for (u64 f : one) for (int q = 0; q < 3; ++q) v.push_back(f);
    g.shuffle(v);
    emit(all, merge_case("merge_window_overflow", make_regions(1024, gid0, {plain, v}, {plain_cnt, {200, 37, 255, 0}}), 1));
  }
  {   // n == region, all distinct, one LDS home: the overflow move's source and destination overlap
    std::set<u64> one;
    while (one.size() < 4096) one.insert(with_lds_home(g, 700, LDS_FP_SLOTS));
    std::vector<u64> v(one.begin(), one.end());
    g.shuffle(v);
    emit(all, merge_case("merge_full_overlap", make_regions(4096, gid0, {plain, v}, {plain_cnt, {1024, 1024, 1024, 1024}}), 1));
  }
  emit(all, merge_case("merge_empty", make_regions(1024, gid0, {plain, {}}, {plain_cnt, {0, 0, 0, 0}}), 1));
  {   // one wave holds every record
    std::vector<u64> d = ordinary(g, 100), v;
    for (int i = 0; i < 256; ++i) v.push_back(d[g.below(d.size())]);
    emit(all, merge_case("merge_uneven_waves", make_regions(1024, gid0, {plain, v}, {plain_cnt, {0, 0, 256, 0}}), 1));
  }
}

// ====================================================================== orig_dedup_plain
struct PlainIn { RegIn reg; u64 slots; std::vector<u64> table; };
struct PlainOut { std::vector<u64> table, newpos; u64 chunk_new = 0, err = 0; };

static PlainOut run_plain(const PlainIn& in) {
  ssc::DevBuf<u64> rfp(in.reg.rfp), table(in.table), newpos(std::vector<u64>(in.reg.nblk * in.reg.region + 1, JUNK));
  ssc::DevBuf<unsigned short> rkey(in.reg.rkey);
  ssc::DevBuf<u32> rcnt(in.reg.rcnt);
  ssc::DevBuf<unsigned long long> ctr(std::vector<unsigned long long>(K_NCTR, 0));
  DedupArgs a{};
  a.rfp = rfp.p; a.rkey = rkey.p; a.rcnt = rcnt.p; a.region = in.reg.region; a.gid0 = in.reg.gid0; a.table = table.p;
  a.table_mask = in.slots - 1; a.newpos = newpos.p; a.ctr = ctr.p;
  hipLaunchKernelGGL((orig_dedup_plain<1, false>), dim3(in.reg.nblk), dim3(BS), 0, 0, a);
  ssc::launched("orig_dedup_plain");
  PlainOut o;
  o.table = table.get(); o.newpos = newpos.get();
  o.chunk_new = ctr.get()[K_CHUNK_NEW]; o.err = ctr.get()[K_ERR];
  o.newpos.resize(o.chunk_new < o.newpos.size() ? o.chunk_new : o.newpos.size());
  return o;
}

static PlainOut play_plain(const PlainIn& in) {
  PlainOut o;
  o.table = in.table;
  const u64 mask = in.slots - 1;
  for (u32 b = 0; b < in.reg.nblk; ++b) {
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
  for (u32 b = 0; b < in.reg.nblk; ++b)
    for (auto& r : records_of(in.reg, b)) {
      if (!before.count(r.fp)) absent.insert(r.fp);
      producer[key_of(in.reg, b, r.lk)] = r.fp;
    }
  if (out.err) return fmt("ctr[K_ERR] = %llx", (unsigned long long)out.err);
  if (out.chunk_new != absent.size()) return fmt("ctr[K_CHUNK_NEW] = %llu, %zu fingerprints were absent", (unsigned long long)out.chunk_new, absent.size());
  if (out.newpos.size() != out.chunk_new) return "fewer records than ctr[K_CHUNK_NEW]";
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

static void plain_cases(std::vector<Report>& all) {
  Rng g(0x5EED0004);
  PlainIn in;
  in.slots = 4096;
  in.table.assign(in.slots, 0);
  const std::vector<u64> A = ordinary(g, 300);
  std::set<u64> one;
  while (one.size() < 24) one.insert(with_lds_home(g, 2044, LDS_FP_SLOTS));   // more than lds_first's window holds
  std::vector<u64> b0(A.begin(), A.begin() + 200), b1(A.begin() + 100, A.end()), b2(A.begin(), A.begin() + 20);
  for (int i = 0; i < 50; ++i) b0.push_back(A[i]);            // repeated inside one workgroup
  for (u64 f : one) { b2.push_back(f); b2.push_back(f); b0.push_back(f); }
  g.shuffle(b0); g.shuffle(b1); g.shuffle(b2);
  for (int i = 150; i < 250; ++i) host_place(in.table, in.slots, 1, A[i], 0);   // already in the table
  { int i = 0; for (u64 f : one) if (i++ % 3 == 0) host_place(in.table, in.slots, 1, f, 0); }
  in.reg = make_regions(4096, (1ull << 34) + 777, {b0, b1, b2},
                        {{100, 0, (u32)b0.size() - 170, 70}, {50, 50, 50, 50}, {(u32)b2.size(), 0, 0, 0}});
  Report r;
  r.name = "dedup_plain_duplicates";
  std::set<u64> fps;
  for (u32 b = 0; b < 3; ++b) for (auto& x : records_of(in.reg, b)) { fps.insert(x.fp); ++r.n; }
  r.distinct = fps.size();
  r.props["max_per_lds_home"] = ssc::WindowModel(fps, LDS_FP_SLOTS, LDS_WIN).max_per_home();
  PlainOut out = g_host_only ? play_plain(in) : run_plain(in);
  const std::string m = check_plain(in, out);
  r.fail(m);
  if (g_host_only && m.empty()) {
    auto chk = [&](const PlainOut& o) { return check_plain(in, o); };
    ssc::try_perturb<PlainOut>(r, ssc::P_DROP, out, chk, [](PlainOut& o) { o.newpos.pop_back(); --o.chunk_new; return true; });
    ssc::try_perturb<PlainOut>(r, ssc::P_DUP, out, chk, [](PlainOut& o) { o.newpos.insert(o.newpos.begin(), o.newpos[0]); ++o.chunk_new; return true; });
    ssc::try_perturb<PlainOut>(r, ssc::P_COUNT_TWICE, out, chk, [](PlainOut& o) { ++o.chunk_new; return true; });
    ssc::try_perturb<PlainOut>(r, ssc::P_SWAP, out, chk, [](PlainOut& o) { std::swap(o.newpos[0], o.newpos[1]); return true; });
  }
  emit(all, r);
}

// ====================================================================== orig_mark + orig_count + orig_scan
struct MarkIn {
  u64 slots = 0, gid0 = 0, chunk_count = 0;
  std::vector<u64> table, newpos;
  std::vector<Rec> prods;   // (fp, key) of every producer
};
struct MarkOut { std::vector<u64> winmask, woff; std::vector<u32> wcnt; u64 chunk_new = 0, err = 0; };

static MarkOut run_mark(const MarkIn& in) {
  const u32 nblk = (u32)((in.chunk_count + BS - 1) / BS);
  ssc::DevBuf<u64> table(in.table), newpos(in.newpos), winmask(std::vector<u64>(in.chunk_count, 0)), woff(std::vector<u64>(nblk, JUNK));
  ssc::DevBuf<u32> wcnt(std::vector<u32>(nblk, 0xEEEEEEEEu));
  std::vector<unsigned long long> c(K_NCTR, 0);
  c[K_INS] = in.newpos.size();
  ssc::DevBuf<unsigned long long> ctr(c);
  MarkArgs a{};
  a.newpos = newpos.p; a.table = table.p; a.gid0 = in.gid0; a.chunk_count = in.chunk_count; a.winmask = winmask.p; a.ww = 1; a.ctr = ctr.p;
  hipLaunchKernelGGL(orig_mark, dim3(2), dim3(BS), 0, 0, a);
  ssc::launched("orig_mark");
  hipLaunchKernelGGL((orig_count<1>), dim3(nblk), dim3(BS), 0, 0, (const u64*)winmask.p, in.chunk_count, wcnt.p);
  ssc::launched("orig_count");
  hipLaunchKernelGGL(orig_scan, dim3(1), dim3(SCAN_BS), 0, 0, (const u32*)wcnt.p, woff.p, nblk, ctr.p);
  ssc::launched("orig_scan");
  MarkOut o;
  o.winmask = winmask.get(); o.woff = woff.get(); o.wcnt = wcnt.get();
  o.chunk_new = ctr.get()[K_CHUNK_NEW]; o.err = ctr.get()[K_ERR];
  return o;
}

static MarkOut play_mark(const MarkIn& in) {
  const u32 nblk = (u32)((in.chunk_count + BS - 1) / BS);
  MarkOut o;
  o.winmask.assign(in.chunk_count, 0); o.wcnt.assign(nblk, 0);
  for (u64 p : in.newpos) {
    const u64 key = ~in.table[2 * p + 1];
    o.winmask[(key >> 8) - in.gid0] |= 1ull << (key & 63);
  }
  for (u64 p = 0; p < in.chunk_count; ++p) o.wcnt[p / BS] += (u32)__builtin_popcountll(o.winmask[p]);
  u64 run = 0;
  for (u32 b = 0; b < nblk; ++b) { o.woff.push_back(run); run += o.wcnt[b]; }
  o.chunk_new = run;
  return o;
}

static std::string check_mark(const MarkIn& in, const MarkOut& out) {
  std::unordered_map<u64, u64> first;   // fp -> its first-found producer (minimum key)
  for (auto& p : in.prods) { auto it = first.find(p.fp); if (it == first.end()) first[p.fp] = p.w; else if (p.w < it->second) it->second = p.w; }
  std::vector<u64> want(in.chunk_count, 0);
  for (auto& f : first) want[(f.second >> 8) - in.gid0] |= 1ull << (f.second & 63);
  if (out.err) return fmt("ctr[K_ERR] = %llx", (unsigned long long)out.err);
  for (u64 p = 0; p < in.chunk_count; ++p)
    if (out.winmask[p] != want[p]) return fmt("parent %llu: winner mask %llx, first-found producers %llx", (unsigned long long)p, (unsigned long long)out.winmask[p], (unsigned long long)want[p]);
  std::vector<u32> cnt((in.chunk_count + BS - 1) / BS, 0);
  for (u64 p = 0; p < in.chunk_count; ++p) cnt[p / BS] += (u32)__builtin_popcountll(want[p]);
  std::vector<u64> off;
  const u64 total = ssc::serial_scan(cnt, off);
  if (out.wcnt != cnt) return "wcnt differs from the winners per workgroup";
  for (size_t b = 0; b < off.size(); ++b)
    if (out.woff[b] != off[b]) return fmt("woff[%zu] = %llu, serial prefix sum %llu", b, (unsigned long long)out.woff[b], (unsigned long long)off[b]);
  if (out.chunk_new != total) return fmt("ctr[K_CHUNK_NEW] = %llu, total %llu", (unsigned long long)out.chunk_new, (unsigned long long)total);
  return "";
}

struct ScanOut { std::vector<u64> woff; u64 total = 0; };
static ScanOut run_scan(const std::vector<u32>& wcnt) {
  ssc::DevBuf<u32> d(wcnt);
  ssc::DevBuf<u64> woff(std::vector<u64>(wcnt.size(), JUNK));
  ssc::DevBuf<unsigned long long> ctr(std::vector<unsigned long long>(K_NCTR, 0));
  hipLaunchKernelGGL(orig_scan, dim3(1), dim3(SCAN_BS), 0, 0, (const u32*)d.p, woff.p, (u32)wcnt.size(), ctr.p);
  ssc::launched("orig_scan");
  return {woff.get(), ctr.get()[K_CHUNK_NEW]};
}
static ScanOut play_scan(const std::vector<u32>& wcnt) {
  ScanOut o;
  for (u32 c : wcnt) { o.woff.push_back(o.total); o.total += c; }
  return o;
}
static std::string check_scan(const std::vector<u32>& wcnt, const ScanOut& out) {
  std::vector<u64> off;
  const u64 total = ssc::serial_scan(wcnt, off);
  if (out.woff.size() != off.size()) return "woff size";
  for (size_t b = 0; b < off.size(); ++b)
    if (out.woff[b] != off[b]) return fmt("woff[%zu] = %llu, serial prefix sum %llu", b, (unsigned long long)out.woff[b], (unsigned long long)off[b]);
  if (out.total != total) return fmt("ctr[K_CHUNK_NEW] = %llu, total %llu", (unsigned long long)out.total, (unsigned long long)total);
  return "";
}

static void mark_scan_cases(std::vector<Report>& all) {
  Rng g(0x5EED0005);
  {
    MarkIn in;
    in.slots = 2048; in.gid0 = (1ull << 35) + 99; in.chunk_count = 3 * BS - 7;
    in.table.assign(2 * in.slots, 0);
    std::set<u64> used;   // (parent, instance) pairs: a producer makes one successor
    Report r;
    r.name = "mark_count_scan";
    for (int i = 0; i < 40; ++i) host_place(in.table, in.slots, 2, g.fp(), ~g.below(in.gid0 << 8));   // older states (keys below gid0): not in newpos
    for (int i = 0; i < 700; ++i) {
      const u64 f = g.fp();
      u64 mn = ~0ull;
      for (u32 q = 0, np = 1 + (u32)g.below(3); q < np; ++q) {
        u64 key;
        // parent 5 produces 64 fingerprints first, the last parent 16, parent 300 nothing
        do {
          const bool fixed = q == 0 && i < 80;
          const u64 parent = fixed ? (i < 64 ? 5 : in.chunk_count - 1) : g.below(in.chunk_count);
          key = ((in.gid0 + parent) << 8) | (fixed && i < 64 ? (u64)i : g.below(64));
        } while ((key >> 8) - in.gid0 == 300 || !used.insert(key).second);
        in.prods.push_back({f, key});
        mn = key < mn ? key : mn;
        ++r.n;
      }
      host_place(in.table, in.slots, 2, f, ~mn);
    }
    for (u64 s = 0; s < in.slots; ++s) if (in.table[2 * s] && (~in.table[2 * s + 1] >> 8) >= in.gid0) in.newpos.push_back(s);
    g.shuffle(in.newpos);
    r.distinct = in.newpos.size();
    MarkOut out = g_host_only ? play_mark(in) : run_mark(in);
    const std::string m = check_mark(in, out);
    r.fail(m);
    if (g_host_only && m.empty()) {
      auto chk = [&](const MarkOut& o) { return check_mark(in, o); };
      ssc::try_perturb<MarkOut>(r, ssc::P_DROP, out, chk, [](MarkOut& o) { for (auto& w : o.winmask) if (w) { w &= w - 1; return true; } return false; });
      ssc::try_perturb<MarkOut>(r, ssc::P_COUNT_TWICE, out, chk, [](MarkOut& o) { ++o.chunk_new; return true; });
      ssc::try_perturb<MarkOut>(r, ssc::P_WOFF, out, chk, [](MarkOut& o) { ++o.woff[1]; return true; });
    }
    emit(all, r);
  }
  for (u32 nblk : {1u, 3u, (u32)SCAN_BS - 1, (u32)SCAN_BS, (u32)SCAN_BS + 1, 3u * SCAN_BS + 5}) {
    std::vector<u32> wcnt(nblk);
    const u32 pick[3] = {0, 1, BS * 64};   // 64 instances per parent: the largest count a workgroup of parents can have at WW = 1
    for (auto& c : wcnt) c = pick[g.below(3)];
    wcnt[nblk - 1] = BS * 64;
    Report r;
    r.name = fmt("scan_nblk_%u", nblk);
    r.n = nblk;
    for (u32 c : wcnt) r.distinct += c;
    r.props["per_thread"] = (nblk + SCAN_BS - 1) / SCAN_BS;
    ScanOut out = g_host_only ? play_scan(wcnt) : run_scan(wcnt);
    const std::string m = check_scan(wcnt, out);
    r.fail(m);
    if (g_host_only && m.empty()) {
      auto chk = [&](const ScanOut& o) { return check_scan(wcnt, o); };
      ssc::try_perturb<ScanOut>(r, ssc::P_WOFF, out, chk, [](ScanOut& o) { ++o.woff.back(); return true; });
      ssc::try_perturb<ScanOut>(r, ssc::P_COUNT_TWICE, out, chk, [](ScanOut& o) { ++o.total; return true; });
    }
    emit(all, r);
  }
}

// ====================================================================== orig_migrate
struct MigIn { int stride; u64 nsrc, dslots; std::vector<u64> src; bool expect_full; };
struct MigOut { std::vector<u64> dst; u64 moved = 0, err = 0; };

template <int STRIDE>
static MigOut run_migrate(const MigIn& in) {
  ssc::DevBuf<u64> src(in.src), dst(std::vector<u64>(STRIDE * in.dslots, 0));
  ssc::DevBuf<unsigned long long> ctr(std::vector<unsigned long long>(K_NCTR, 0)), moved(std::vector<unsigned long long>(1, 0));
  const u64 groups = in.nsrc / (4 / STRIDE);
  hipLaunchKernelGGL((orig_migrate<STRIDE>), dim3((unsigned)((groups + BS - 1) / BS)), dim3(BS), 0, 0, (const u64*)src.p, in.nsrc, dst.p,
                     in.dslots - 1, ctr.p, moved.p);
  ssc::launched("orig_migrate");
  return {dst.get(), moved.get()[0], ctr.get()[K_ERR]};
}
static MigOut play_migrate(const MigIn& in) {
  MigOut o;
  const u64 st = in.stride, mask = in.dslots - 1;
  o.dst.assign(st * in.dslots, 0);
  for (u64 e = 0; e < in.nsrc; ++e) {
    const u64 f = in.src[st * e];
    if (!f) continue;
    ++o.moved;
    u64 s = f & mask, k = 0;
    for (; k < in.dslots && o.dst[st * s]; ++k) s = (s + 1) & mask;
    if (k == in.dslots) { o.err |= OE_TABLE_FULL; continue; }
    o.dst[st * s] = f;
    if (st == 2) o.dst[2 * s + 1] = in.src[2 * e + 1];
  }
  return o;
}
static std::string check_migrate(const MigIn& in, const MigOut& out) {
  const u64 st = in.stride;
  std::unordered_map<u64, u64> want;
  for (u64 e = 0; e < in.nsrc; ++e) if (in.src[st * e]) want[in.src[st * e]] = st == 2 ? in.src[2 * e + 1] : 0;
  std::set<u64> got;
  for (u64 s = 0; s < in.dslots; ++s) {
    const u64 f = out.dst[st * s];
    if (!f) continue;
    auto it = want.find(f);
    if (it == want.end()) return fmt("destination slot %llu holds %016llx, which the source does not", (unsigned long long)s, (unsigned long long)f);
    if (!got.insert(f).second) return fmt("fingerprint %016llx moved twice", (unsigned long long)f);
    if (st == 2 && out.dst[2 * s + 1] != it->second) return fmt("fingerprint %016llx: key word %llx, source %llx", (unsigned long long)f, (unsigned long long)out.dst[2 * s + 1], (unsigned long long)it->second);
  }
  if (in.expect_full) {
    if (!(out.err & OE_TABLE_FULL)) return fmt("ctr[K_ERR] = %llx, OE_TABLE_FULL expected", (unsigned long long)out.err);
    return "";
  }
  if (out.err) return fmt("ctr[K_ERR] = %llx", (unsigned long long)out.err);
  if (got.size() != want.size()) return fmt("%zu of %zu entries arrived", got.size(), want.size());
  if (out.moved != want.size()) return fmt("moved = %llu, %zu entries", (unsigned long long)out.moved, want.size());
  return "";
}

static void migrate_cases(std::vector<Report>& all) {
  Rng g(0x5EED0006);
  for (int stride : {1, 2})
    for (bool full : {false, true}) {
      MigIn in;
      in.stride = stride; in.expect_full = full;
      in.nsrc = 1024; in.dslots = full ? 512 : 2048;
      in.src.assign(stride * in.nsrc, 0);
      const u64 count = full ? 513 : 512, home = 1000;
      std::set<u64> fps;
      // one source cluster from slot 1000 across the table's end; in a 2^11-slot destination the entries
      // share the two home slots 1000 and 2024 (the second cluster wraps there too)
      while (fps.size() < count) fps.insert((g.next() & ~2047ull) | home | ((g.next() & 1) << 10));
      u64 s = home;
      for (u64 f : fps) { in.src[stride * s] = f; if (stride == 2) in.src[2 * s + 1] = ~rand_key(g); s = (s + 1) & (in.nsrc - 1); }
      Report r;
      r.name = fmt("migrate%d_%s", stride, full ? "full" : "cluster");
      r.n = r.distinct = count;
      r.props["src_wraps"] = in.src[stride * (in.nsrc - 1)] != 0 && in.src[0] != 0;
      r.props["dst_slots"] = (long long)in.dslots;
      MigOut out = g_host_only ? play_migrate(in) : (stride == 1 ? run_migrate<1>(in) : run_migrate<2>(in));
      const std::string m = check_migrate(in, out);
      r.fail(m);
      if (g_host_only && m.empty() && !full) {
        auto chk = [&](const MigOut& o) { return check_migrate(in, o); };
        const u64 st = stride;
        ssc::try_perturb<MigOut>(r, ssc::P_DROP, out, chk, [&](MigOut& o) { for (u64 q = 0; q < in.dslots; ++q) if (o.dst[st * q]) { o.dst[st * q] = 0; return true; } return false; });
        ssc::try_perturb<MigOut>(r, ssc::P_DUP, out, chk, [&](MigOut& o) {
          u64 from = 0; while (!o.dst[st * from]) ++from;
          u64 to = 0; while (o.dst[st * to]) ++to;
          for (u64 q = 0; q < st; ++q) o.dst[st * to + q] = o.dst[st * from + q];
          return true; });
        if (stride == 2)
          ssc::try_perturb<MigOut>(r, ssc::P_KEY_RAISED, out, chk, [&](MigOut& o) { for (u64 q = 0; q < in.dslots; ++q) if (o.dst[2 * q]) { o.dst[2 * q + 1] -= 1; return true; } return false; });
        ssc::try_perturb<MigOut>(r, ssc::P_COUNT_TWICE, out, chk, [](MigOut& o) { ++o.moved; return true; });
      }
      emit(all, r);
    }
}

// ====================================================================== orig_route_blk
struct RouteIn { RegIn reg; u32 world; u64 cap; };
struct RouteOut { std::vector<u64> route; std::vector<unsigned long long> cnt; };

static RouteOut run_route(const RouteIn& in) {
  ssc::DevBuf<u64> rfp(in.reg.rfp), route(std::vector<u64>(in.world * in.cap * 2, 0));
  ssc::DevBuf<unsigned short> rkey(in.reg.rkey);
  ssc::DevBuf<u32> rcnt(in.reg.rcnt);
  ssc::DevBuf<unsigned long long> cnt(std::vector<unsigned long long>(in.world, 0));
  RouteArgs a{};
  a.rfp = rfp.p; a.rkey = rkey.p; a.rcnt = rcnt.p; a.region = in.reg.region; a.route = route.p; a.route_cap = in.cap; a.world = in.world; a.rcnt_out = cnt.p;
  hipLaunchKernelGGL(orig_route_blk, dim3(in.reg.nblk), dim3(BS), 0, 0, a);
  ssc::launched("orig_route_blk");
  return {route.get(), cnt.get()};
}
static u64 route_word(u32 b, u32 lk) { return (((u64)b * BS + (lk >> 8)) << 8) | (u64)(lk & 255u); }
static RouteOut play_route(const RouteIn& in) {
  RouteOut o;
  o.route.assign(in.world * in.cap * 2, 0); o.cnt.assign(in.world, 0);
  for (u32 b = 0; b < in.reg.nblk; ++b) {
    std::set<u64> here;
    for (auto& r : records_of(in.reg, b)) {
      if (!here.insert(r.fp).second) continue;
      const u32 w = fp_owner(r.fp, in.world);
      o.route[(w * in.cap + o.cnt[w]) * 2] = r.fp;
      o.route[(w * in.cap + o.cnt[w]) * 2 + 1] = route_word(b, r.lk);
      ++o.cnt[w];
    }
  }
  return o;
}
static std::string check_route(const RouteIn& in, const RouteOut& out) {
  std::unordered_map<u64, u64> producer;   // slot word -> fp
  std::vector<std::set<u64>> fps(in.reg.nblk);
  std::set<u64> every, routed;
  for (u32 b = 0; b < in.reg.nblk; ++b)
    for (auto& r : records_of(in.reg, b)) { producer[route_word(b, r.lk)] = r.fp; fps[b].insert(r.fp); every.insert(r.fp); }
  std::vector<ssc::WindowModel> win;
  for (u32 b = 0; b < in.reg.nblk; ++b) win.emplace_back(fps[b], ROUTE_FP_SLOTS, LDS_WIN);
  std::set<std::pair<u64, u64>> once;   // (workgroup, fp)
  std::set<u64> words;
  for (u32 w = 0; w < in.world; ++w) {
    if (out.cnt[w] > in.cap) return fmt("owner %u: count %llu beyond the segment", w, out.cnt[w]);
    for (u64 i = 0; i < in.cap; ++i) {
      const u64 f = out.route[(w * in.cap + i) * 2], word = out.route[(w * in.cap + i) * 2 + 1];
      if (i >= out.cnt[w]) {
        if (f) return fmt("owner %u: a record was written at %llu, beyond its count %llu", w, (unsigned long long)i, out.cnt[w]);
        continue;
      }
      auto it = producer.find(word);
      if (it == producer.end() || it->second != f) return fmt("owner %u record %llu: slot word %llx is no producer of %016llx", w, (unsigned long long)i, (unsigned long long)word, (unsigned long long)f);
      if (fp_owner(f, in.world) != w) return fmt("fingerprint %016llx sits in owner %u's segment, its owner is %u", (unsigned long long)f, w, fp_owner(f, in.world));
      if (!words.insert(word).second) return fmt("slot word %llx routed twice", (unsigned long long)word);
      const u64 b = (word >> 8) / BS;
      if (!once.insert({b, f}).second && !win[b].may_be_full(f))
        return fmt("workgroup %llu routed %016llx twice although its window cannot have been full", (unsigned long long)b, (unsigned long long)f);
      routed.insert(f);
    }
  }
  if (routed != every) return fmt("%zu of %zu distinct fingerprints were routed", routed.size(), every.size());
  return "";
}

static void route_cases(std::vector<Report>& all) {
  Rng g(0x5EED0007);
  const std::vector<u64> A = ordinary(g, 400);
  std::set<u64> one;
  while (one.size() < 20) one.insert(with_lds_home(g, 4093, ROUTE_FP_SLOTS));
  std::vector<u64> b0(A.begin(), A.begin() + 250), b1(A.begin() + 150, A.end()), b2;
  for (int i = 0; i < 120; ++i) b0.push_back(A[g.below(250)]);
  for (u64 f : one) { b2.push_back(f); b2.push_back(f); b1.push_back(f); }
  g.shuffle(b0); g.shuffle(b1); g.shuffle(b2);
  for (u32 world : {1u, 2u, 3u, 8u}) {
    RouteIn in;
    in.world = world;
    in.reg = make_regions(4096, 0, {b0, b1, b2}, {{120, 250, 0, 0}, {0, 70, 100, (u32)b1.size() - 170}, {10, 10, 10, 10}});
    in.cap = b0.size() + b1.size() + b2.size();
    Report r;
    r.name = fmt("route_world_%u", world);
    std::set<u64> fps;
    for (u32 b = 0; b < 3; ++b) for (auto& x : records_of(in.reg, b)) { fps.insert(x.fp); ++r.n; }
    r.distinct = fps.size();
    RouteOut out = g_host_only ? play_route(in) : run_route(in);
    const std::string m = check_route(in, out);
    r.fail(m);
    if (g_host_only && m.empty()) {
      auto chk = [&](const RouteOut& o) { return check_route(in, o); };
      ssc::try_perturb<RouteOut>(r, ssc::P_DROP, out, chk, [](RouteOut& o) { --o.cnt[0]; return true; });
      ssc::try_perturb<RouteOut>(r, ssc::P_DUP, out, chk, [&](RouteOut& o) {
        for (int q = 0; q < 2; ++q) o.route[o.cnt[0] * 2 + q] = o.route[q];
        ++o.cnt[0];
        return true; });
      ssc::try_perturb<RouteOut>(r, ssc::P_COUNT_TWICE, out, chk, [](RouteOut& o) { ++o.cnt[0]; return true; });
    }
    emit(all, r);
  }
}

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    if (!std::strcmp(argv[i], "--host-only")) g_host_only = true;
    else { std::fprintf(stderr, "usage: orig_seen_set_check [--host-only]\n"); return 64; }
  }
  std::vector<Report> all;
  probe_cases(false, all);
  probe_cases(true, all);
  merge_cases(all);
  plain_cases(all);
  mark_scan_cases(all);
  migrate_cases(all);
  route_cases(all);
  bool ok = true;
  for (auto& r : all) ok &= r.first.empty();
  return ok ? 0 : 1;
}
