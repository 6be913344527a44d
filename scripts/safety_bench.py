#!/usr/bin/env python3
"""Measurements of the log- and commit-safety invariants for raft_original (bench.py
itself is the C2 search with the two old invariants and is only run here, never changed).

  scripts/safety_bench.py [--parts cost bench] [--parent DIR] [--out profiles/orig_safety.json]   (on an MI355X)

  cost  C2 (configs/c2.cfg) and configs/c2_md6.cfg, -workers N: the search with the cfg's two invariants
        (the kernels compiled without the safety code) and with all eleven (the WithSafety
        instantiations), the two handles alternating in one process after a warm-up run each: counts
        (equal), the median mc_run time and the per-kernel split.
  bench bench.py's C2 line by this tree and by the parent's (DIR: a checkout of the parent commit with
        its package built), alternating, --rounds times each.
Each part runs in a child process of its own (one GPU process at a time).  The compiler's resource
report of both instantiations of the kernels that check invariants (scripts/check_isa.py over the built
library, C2's shape) goes into the same file.
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
SAFETY_TLA = os.path.join(CONFIGS, "raft_original_safety_mc.tla")
SAFETY = ["CommitWithinLog", "LeaderVotesQuorum", "CandidateTermNotInLog", "LeaderHasLatestOfTerm", "VotesGrantedInv",
          "QuorumLogInv", "MoreUpToDateCorrect", "LeaderCompleteness", "StateMachineSafety"]
CHECKED = ("orig_generate", "orig_generate_lead", "orig_generate_sym", "orig_materialize", "orig_materialize_plain",
           "orig_materialize_sh", "orig_simulate")


def with_safety(cfg):
    fd, path = tempfile.mkstemp(suffix=".cfg")
    with os.fdopen(fd, "w") as f:
        f.write(open(cfg).read().rstrip("\n") + "\n" + "".join("    %s\n" % n for n in SAFETY))
    return path


def counts(r):
    return {"verdict": r.verdict, "generated": r.generated, "distinct": r.distinct, "depth": r.depth}


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


def part_cost(mod, a):
    doc = {}
    for name, sizes in (("c2", dict(fp_table_bytes=4 << 30, state_store_bytes=16 << 30)),
                        ("c2_md6", dict(fp_table_bytes=8 << 30, state_store_bytes=64 << 30))):   # bench.py's variants.c2_md6 sizes
        base = os.path.join(CONFIGS, name + ".cfg")
        cfg = with_safety(base)
        d = {"sizes": sizes, "workers": 0}
        try:
            with mod.ModelChecker(TLA, base, workers=0, **sizes) as two, mod.ModelChecker(SAFETY_TLA, cfg, workers=0, **sizes) as eleven:
                runs = {"two": [], "eleven": []}
                for k in range(a.warmup + a.repeats):
                    for which, mc in (("two", two), ("eleven", eleven)):
                        r, t = timed(mc)
                        assert r.verdict == "OK", (which, r.violated, r.error)
                        assert d.setdefault("counts", counts(r)) == counts(r)
                        if k >= a.warmup:
                            runs[which].append(t)
                for which in runs:
                    d[which] = median_of(runs[which])
        finally:
            os.unlink(cfg)
        doc[name] = d
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


def resources(shape="3,2,3,2,5"):
    """registers, scratch and instructions of both instantiations of every kernel that checks invariants, one shape"""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import check_isa
    out = {}
    for co in check_isa.code_objects(check_isa.DEFAULT):
        for k, v in check_isa.kernels(co).items():
            name = next((n for n in sorted(CHECKED, key=len, reverse=True) if "_ZN3rmc%d%sI" % (len(n), n) in k), None)
            if not name or "OrigILi" not in k or k.split("OrigILi")[1].split("EEE")[0].replace("ELi", ",") != shape:
                continue
            regs = v["vgprs"]
            out.setdefault(name, {})["with_safety" if "WithSafety" in k else "plain"] = {
                "vgprs": regs, "agprs": v["agprs"], "scratch_bytes": v["scratch_bytes"], "lds_bytes": v["lds_bytes"],
                "instructions": v["instructions"], "waves_per_simd": max(1, min(8, 512 // max(regs, 1)))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", nargs="+", default=["cost", "bench"])
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
        print(json.dumps({"cost": part_cost}[a.worker](mod, a)))
        return
    doc = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {}
    doc["resources_c2_shape"] = resources()
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
        if a.out:
            with open(a.out, "w") as f:
                f.write(json.dumps(doc, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
