#!/usr/bin/env python3
"""Measurements of the action properties for raft_original (bench.py itself is the C2
search without properties and is only run here, never changed).

  scripts/actions_bench.py [--parts cost sim bench] [--parent DIR] [--out profiles/orig_actions.json]   (on an MI355X)

  cost  C2 (configs/c2.cfg), -workers N: the search without PROPERTIES (the kernels compiled without the
        property code) and with all five Raft properties (the WithActions instantiations), the two handles
        alternating in one process after a warm-up run each: counts (equal), the median mc_run time and
        the per-kernel split.
  sim   orig_simulate on configs/c2.cfg, 2^20 walks of depth 64, without and with the five, the same way.
  bench bench.py's C2 line by this tree and by the parent's (DIR: a checkout of the parent commit with
        its package built), alternating, --rounds times each.
Each part runs in a child process of its own (one GPU process at a time).  Two resource reports of every
instantiation of the four kernels that check properties, C2's shape and (5,2,3,3,8), go into the same file:
  resources_isa       scripts/check_isa.py over the built library: registers, scratch, LDS, instructions;
  resources_compiler  with --remarks LOG, the compiler's own report (VGPRs, spilled VGPRs, scratch, waves per
                      SIMD under the kernel's occupancy hint) parsed from the output of a build of
                      csrc/orig_backend.hip with -Rpass-analysis=kernel-resource-usage added to HIPFLAGS;
                      --hint4-remarks LOG the same for a build with WithActions' hints left at 4 waves (the
                      spills that made them 3).  Without the option the key already in --out is kept.
If a listed property turns out violated on c2.cfg it is dropped from the timed list and named under
"dropped": a run that stops early is no cost measurement.
"""
import argparse
import importlib
import re
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, "configs")
TLA = os.path.join(CONFIGS, "raft_original_mc.tla")
ACTIONS_TLA = os.path.join(CONFIGS, "raft_original_actions_mc.tla")
FIVE = ["TermsMonotonic", "OneVotePerTerm", "LeaderAppendOnly", "CommittedNeverLost", "CommitIndexMonotonic"]
CHECKED = ("orig_generate", "orig_generate_lead", "orig_generate_sym", "orig_simulate")
SHAPES = ("3,2,3,2,5", "5,2,3,3,8")
C2_SIZES = dict(fp_table_bytes=4 << 30, state_store_bytes=16 << 30)


def with_properties(cfg, names=FIVE):
    fd, path = tempfile.mkstemp(suffix=".cfg")
    with os.fdopen(fd, "w") as f:
        f.write(open(cfg).read().rstrip("\n") + "\nPROPERTIES\n" + "".join("    %s\n" % n for n in names))
    return path


def holding_on(mod, base, run, **kw):
    """FIVE minus the properties `run` finds violated on the cfg `base`: (cfg path with the rest, the rest, the dropped)"""
    names, dropped = list(FIVE), []
    while True:
        cfg = with_properties(base, names)
        with mod.ModelChecker(ACTIONS_TLA, cfg, **kw) as mc:
            r = run(mc)
        if r.verdict != "ACTION_PROPERTY_VIOLATION":
            assert r.verdict == "OK", (r.verdict, r.violated, r.error)
            return cfg, names, dropped
        os.unlink(cfg)
        names.remove(r.violated)
        dropped.append(r.violated)


def counts(r):
    return {"verdict": r.verdict, "generated": r.generated, "distinct": r.distinct, "depth": r.depth}


def timed(run):
    t0 = time.perf_counter()
    r = run()   # returns after the run's last device synchronise
    return r, {"seconds_total": r.seconds, "seconds_kernels": r.kernel_seconds, "wall_s": time.perf_counter() - t0,
               "kernels_ms": {n: v["ms"] for n, v in r.kernels.items()}}


def median_of(runs):
    out = {k: statistics.median(x[k] for x in runs) for k in ("seconds_total", "seconds_kernels", "wall_s")}
    out["kernels_ms"] = {n: statistics.median(x["kernels_ms"][n] for x in runs) for n in runs[0]["kernels_ms"]}
    out["repeats"] = len(runs)
    return out


def alternate(a, handles, run, what):
    """handles: {"none": mc, "five": mc}; run(mc) -> Result; the two alternate, a.warmup + a.repeats times each"""
    d, runs = {}, {k: [] for k in handles}
    for k in range(a.warmup + a.repeats):
        for which, mc in handles.items():
            r, t = timed(lambda: run(mc))
            assert r.verdict == "OK", (which, r.violated, r.error)
            assert d.setdefault("counts", what(r)) == what(r), (which, what(r))
            if k >= a.warmup:
                runs[which].append(t)
    for which in runs:
        d[which] = median_of(runs[which])
    return d


def part_cost(mod, a):
    base = os.path.join(CONFIGS, "c2.cfg")
    cfg, names, dropped = holding_on(mod, base, lambda mc: mc.run(), workers=0, **C2_SIZES)
    try:
        with mod.ModelChecker(TLA, base, workers=0, **C2_SIZES) as none, mod.ModelChecker(ACTIONS_TLA, cfg, workers=0, **C2_SIZES) as five:
            d = alternate(a, {"none": none, "five": five}, lambda mc: mc.run(), counts)
    finally:
        os.unlink(cfg)
    d.update(sizes=C2_SIZES, workers=0, properties=names, dropped=dropped)
    return {"c2": d}


def part_sim(mod, a):
    base = os.path.join(CONFIGS, "c2.cfg")
    cfg, names, dropped = holding_on(mod, base, lambda mc: mc.simulate(1 << 20, 1 << 20), seed=1, max_depth=64)
    try:
        with mod.ModelChecker(TLA, base, seed=1, max_depth=64) as none, mod.ModelChecker(ACTIONS_TLA, cfg, seed=1, max_depth=64) as five:
            d = alternate(a, {"none": none, "five": five}, lambda mc: mc.simulate(1 << 20, 1 << 20),
                          lambda r: {"verdict": r.verdict, "generated": r.generated, "steps": r.steps, "walks": r.walks})
    finally:
        os.unlink(cfg)
    d.update(walks=1 << 20, depth=64, seed=1, properties=names, dropped=dropped)
    return {"c2": d}


def part_bench(a):
    trees = {"this": ROOT, "parent": os.path.abspath(a.parent)}
    lines = {k: [] for k in trees}
    for _ in range(a.rounds):
        for name, tree in trees.items():
            p = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(a.steps), "--warmup", "1",
                                "--no-cpu-baseline", "--no-extra"], capture_output=True, text=True, timeout=900, cwd=tree)
            if p.returncode != 0:
                raise SystemExit("bench.py of %s failed: %s" % (tree, p.stderr[-2000:]))
            lines[name].append(json.loads(p.stdout.strip().splitlines()[-1]))
    doc = {"steps": a.steps, "rounds": a.rounds}
    for name, ls in lines.items():
        ms = [x["ms_per_step"] for x in ls]
        doc[name] = {"ms_per_step": ms, "median_ms_per_step": statistics.median(ms), "spread_ms": max(ms) - min(ms)}
    # the requirement: this tree's median inside the parent's own min-max spread (below its minimum: faster)
    med, lo, hi = doc["this"]["median_ms_per_step"], min(doc["parent"]["ms_per_step"]), max(doc["parent"]["ms_per_step"])
    doc["this_median_inside_parent_spread"] = lo <= med <= hi
    doc["this_median_at_most_parent_max"] = med <= hi
    return doc


def resources():
    """registers, scratch and instructions of every instantiation of the four kernels, per shape"""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import check_isa
    out = {}
    for co in check_isa.code_objects(check_isa.DEFAULT):
        for k, v in check_isa.kernels(co).items():
            name = next((n for n in sorted(CHECKED, key=len, reverse=True) if "_ZN3rmc%d%sI" % (len(n), n) in k), None)
            if not name or "OrigILi" not in k:
                continue
            shape = k.split("OrigILi")[1].split("EEE")[0].replace("ELi", ",")
            if shape not in SHAPES:
                continue
            inst = ("WithActions<WithSafety<S>>" if "WithActions" in k and "WithSafety" in k else "WithActions<S>" if "WithActions" in k
                    else "WithSafety<S>" if "WithSafety" in k else "S")
            out.setdefault(shape, {}).setdefault(name, {})[inst] = {
                "vgprs": v["vgprs"], "agprs": v["agprs"], "scratch_bytes": v["scratch_bytes"], "lds_bytes": v["lds_bytes"],
                "instructions": v["instructions"]}
    return out


def compiler_resources(log):
    """the same kernels from the compiler's -Rpass-analysis=kernel-resource-usage remarks of a build: the
    occupancy is the compiler's, under the kernel's amdgpu_waves_per_eu hint"""
    out = {}
    for b in re.split(r"remark: [^\n]*Function Name: ", open(log).read())[1:]:
        k = b.split("\n")[0].strip()
        name = next((n for n in sorted(CHECKED, key=len, reverse=True) if "_ZN3rmc%d%sI" % (len(n), n) in k), None)
        if not name or "OrigILi" not in k:
            continue
        shape = k.split("OrigILi")[1].split("EEE")[0].replace("ELi", ",")
        if shape not in SHAPES:
            continue
        inst = ("WithActions<WithSafety<S>>" if "WithActions" in k and "WithSafety" in k else "WithActions<S>" if "WithActions" in k
                else "WithSafety<S>" if "WithSafety" in k else "S")

        def num(key):
            m = re.search(key + r": (\d+)", b)
            return int(m.group(1)) if m else None
        out.setdefault(shape, {}).setdefault(name, {})[inst] = {
            "vgprs": num("VGPRs"), "vgprs_spilled": num("VGPRs Spill"), "scratch_bytes": num(r"ScratchSize \[bytes/lane\]"),
            "waves_per_simd": num(r"Occupancy \[waves/SIMD\]")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", nargs="*", default=["cost", "sim", "bench"], help="none: the resource reports only")
    ap.add_argument("--parent", help="checkout of the parent commit with raft-tla_amd/_build/libraftmc.so built (part bench)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--remarks", help="compiler output of a build with -Rpass-analysis=kernel-resource-usage")
    ap.add_argument("--hint4-remarks", help="the same for a build with WithActions' occupancy hints at 4 waves")
    ap.add_argument("--worker", help="(internal) run one part in this process and print its JSON")
    a = ap.parse_args()
    if a.worker:
        sys.path.insert(0, ROOT)
        mod = importlib.import_module("raft-tla_amd")
        print(json.dumps({"cost": part_cost, "sim": part_sim}[a.worker](mod, a)))
        return
    doc = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {}
    doc["resources_isa"] = resources()
    if a.remarks:
        doc["resources_compiler"] = compiler_resources(a.remarks)
    if a.hint4_remarks:
        doc["resources_compiler_hint4"] = {s: {k: {i: x for i, x in v.items() if i.startswith("WithActions")} for k, v in ks.items()}
                                           for s, ks in compiler_resources(a.hint4_remarks).items()}
    def save():
        if a.out:
            with open(a.out, "w") as f:
                f.write(json.dumps(doc, indent=1, sort_keys=True) + "\n")
    save()
    for part in a.parts:
        if part == "bench":
            if not a.parent or not os.path.exists(os.path.join(a.parent, "raft-tla_amd", "_build", "libraftmc.so")):
                raise SystemExit("--parent DIR: a checkout of the parent commit with its library built")
            doc["bench_c2"] = part_bench(a)
        else:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", part, "--warmup", str(a.warmup), "--repeats", str(a.repeats)],
                               capture_output=True, text=True, timeout=1100)
            if p.returncode != 0:
                raise SystemExit("part %s failed: %s" % (part, p.stderr[-3000:]))
            doc[part] = json.loads(p.stdout.strip().splitlines()[-1])
        print(part, json.dumps(doc.get(part, doc.get("bench_c2")))[:1500], flush=True)
        save()


if __name__ == "__main__":
    main()
