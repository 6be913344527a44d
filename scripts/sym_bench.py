#!/usr/bin/env python3
"""Measurements of SYMMETRY Permutations(Server) for raft_original (bench.py itself is
the unsymmetric C2 search and is only run here, never changed).

  scripts/sym_bench.py [--parts c2 c5e c5v2 bench] [--parent DIR] [--out profiles/orig_symmetry.json]   (on an MI355X)

  c2    C2 (configs/c2.cfg) with and without `SYMMETRY ServerSymmetry`, the two handles alternating in
        one process after a warm-up run each: counts and the median mc_run time.  The symmetric counts
        are checked once against the generated path (TLC's rule) on the GPU with the same cfg
        (_build/tlagen_co/c2_sym.gen.hip, built by csrc/tlagen/prebuild.py).
  c5e   configs/c5e_noleader.cfg with SYMMETRY, -workers 1: the stop point of the first 5-server
        election (depth 14 as without symmetry), its counters, the time, the seen-set and store it was
        given, and the oracle's check-trace of the counterexample against the cfg WITHOUT the line.
  c5v2  configs/c5v2.cfg with SYMMETRY to depth 12, -workers N: distinct against the unsymmetric
        482,207,085, and the time.
  bench bench.py's C2 line by this tree and by the parent's (DIR: a checkout of the parent commit with
        its package built), alternating, --rounds times each.
Each part runs in a child process of its own (one GPU process at a time).  The compiler's resource
report of orig_generate_sym (scripts/check_isa.py over the built library) goes into the same file.
"""
import argparse
import importlib
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
SYM_TLA = os.path.join(CONFIGS, "raft_original_sym_mc.tla")
C5V2_D12_UNSYMMETRIC = 482207085


def with_symmetry(cfg):
    fd, path = tempfile.mkstemp(suffix=".cfg")
    with os.fdopen(fd, "w") as f:
        f.write(open(cfg).read() + "\nSYMMETRY ServerSymmetry\n")
    return path


def counts(r):
    return {"verdict": r.verdict, "generated": r.generated, "distinct": r.distinct, "depth": r.depth, "left_on_queue": r.left_on_queue}


def timed(mc):
    t0 = time.perf_counter()
    r = mc.run()   # returns after the run's last device synchronise
    return r, {"seconds_total": r.seconds, "seconds_kernels": r.kernel_seconds, "wall_s": time.perf_counter() - t0,
               "kernels_ms": {n: v["ms"] for n, v in r.kernels.items()}}


def median_of(runs):
    out = {k: statistics.median(x[k] for x in runs) for k in ("seconds_total", "seconds_kernels", "wall_s")}
    out["kernels_ms"] = {n: statistics.median(x["kernels_ms"][n] for x in runs) for n in runs[0]["kernels_ms"]}
    out["repeats"] = len(runs)
    return out


def part_c2(mod, a):
    sizes = dict(fp_table_bytes=4 << 30, state_store_bytes=16 << 30)
    sym_cfg = os.path.join(CONFIGS, "c2_sym.cfg")
    doc = {"sizes": sizes, "workers": 0}
    with mod.ModelChecker(TLA, os.path.join(CONFIGS, "c2.cfg"), workers=0, **sizes) as plain, \
            mod.ModelChecker(SYM_TLA, sym_cfg, workers=0, **sizes) as sym:
        runs = {"plain": [], "symmetric": []}
        for k in range(a.warmup + a.repeats):
            for name, mc in (("plain", plain), ("symmetric", sym)):
                r, t = timed(mc)
                assert r.verdict == "OK", r.error
                assert doc.setdefault(name + "_counts", counts(r)) == counts(r)
                if k >= a.warmup:
                    runs[name].append(t)
        for name in runs:
            doc[name] = median_of(runs[name])
    gen = os.path.join(ROOT, "raft-tla_amd", "_build", "tlagen_co", "c2_sym.gen.hip")
    with mod.ModelChecker(gen, sym_cfg, frontend="generated", workers=0, fp_table_bytes=1 << 30, state_store_bytes=64 << 30) as mc:
        r, t = timed(mc)
    doc["generated_path_counts"], doc["generated_path_seconds_total"] = counts(r), t["seconds_total"]
    doc["generated_path_levels"] = [lv[0] for lv in r.levels]
    for f in ("verdict", "generated", "distinct", "depth"):
        assert doc["symmetric_counts"][f] == doc["generated_path_counts"][f], (doc["symmetric_counts"], doc["generated_path_counts"])
    return doc


def part_c5e(mod, a):
    plain = os.path.join(CONFIGS, "c5e_noleader.cfg")
    cfg = with_symmetry(plain)
    sizes = dict(fp_table_bytes=2 << 30, state_store_bytes=8 << 30)
    try:
        with mod.ModelChecker(SYM_TLA, cfg, workers=1, **sizes) as mc:
            slot = mc.describe()["state_bytes_stored"] + 8
            runs = []
            for k in range(a.warmup + a.repeats):
                r, t = timed(mc)
                if k >= a.warmup:
                    runs.append(t)
    finally:
        os.unlink(cfg)
    assert (r.verdict, r.violated, r.depth) == ("INVARIANT_VIOLATION", "NoLeader", 14), (r, r.error)
    states = [" ".join(blk.split("\n")[1:]) for blk in r.trace_text.strip().split("\n\n")]
    with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
        f.write("\n".join(states) + "\n")
    out = subprocess.run([os.path.join(ROOT, "oracle", "_build", "raft_oracle"), "check-trace", "--tla", TLA, "--cfg", plain,
                          "--golden", f.name], capture_output=True, text=True, timeout=600).stdout
    os.unlink(f.name)
    o = json.loads(out.strip().splitlines()[-1])
    assert o["valid"] and o["violated"] == "NoLeader" and o["length"] == 14, o
    doc = {"sizes": sizes, "workers": 1, "counts": counts(r), "actions": r.actions, "levels": [lv[0] for lv in r.levels],
           "seen_set_bytes_needed": r.distinct * 16, "store_bytes_needed": r.distinct * slot, "check_trace": o}
    doc.update(median_of(runs))
    return doc


def part_c5v2(mod, a):
    cfg = with_symmetry(os.path.join(CONFIGS, "c5v2.cfg"))
    sizes = dict(fp_table_bytes=4 << 30, state_store_bytes=32 << 30)
    try:
        with mod.ModelChecker(SYM_TLA, cfg, workers=0, max_depth=12, **sizes) as mc:
            runs = []
            for k in range(a.warmup + a.repeats):
                r, t = timed(mc)
                if k >= a.warmup:
                    runs.append(t)
    finally:
        os.unlink(cfg)
    assert r.verdict == "DEPTH_LIMIT", (r, r.error)
    doc = {"sizes": sizes, "workers": 0, "max_depth": 12, "counts": counts(r), "levels": [lv[0] for lv in r.levels],
           "unsymmetric_distinct": C5V2_D12_UNSYMMETRIC, "reduction": C5V2_D12_UNSYMMETRIC / r.distinct}
    doc.update(median_of(runs))
    return doc


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
    return doc


def resources():
    """orig_generate_sym's registers, scratch and LDS as the compiler reports them, per compiled shape"""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import check_isa
    out = {}
    for co in check_isa.code_objects(check_isa.DEFAULT):
        for k, v in check_isa.kernels(co).items():
            if "orig_generate_sym" not in k:
                continue
            shape = k.split("OrigILi")[1].split("EEEEE")[0].replace("ELi", ",")
            regs = v["vgprs"]   # arch + accumulation registers of one lane; 512 per SIMD lane, 8 waves at most
            out[shape] = {"vgprs_total": regs, "agprs": v["agprs"], "scratch_bytes": v["scratch_bytes"], "dynamic_stack": v["dynamic_stack"],
                          "lds_bytes": v["lds_bytes"], "instructions": v["instructions"], "waves_per_simd": max(1, min(8, 512 // max(regs, 1)))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", nargs="+", default=["c2", "c5e", "c5v2", "bench"])
    ap.add_argument("--parent", help="checkout of the parent commit with raft-tla_amd/_build/libraftmc.so built (part bench)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", help="(internal) run one part in this process and print its JSON")
    a = ap.parse_args()
    if a.worker:
        sys.path.insert(0, ROOT)
        mod = importlib.import_module("raft-tla_amd")
        print(json.dumps({"c2": part_c2, "c5e": part_c5e, "c5v2": part_c5v2}[a.worker](mod, a)))
        return
    doc = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {}
    doc["resources_orig_generate_sym"] = resources()
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
        print(part, json.dumps(doc.get(part, doc.get("bench_c2")))[:600], flush=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write(json.dumps(doc, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
