#!/usr/bin/env python3
"""Measurements of the simulation mode (bench.py is the BFS's and is not involved).

  scripts/sim_bench.py --out profiles/sim_c2.json            (on an MI355X)
      c2.cfg, 2^20 walks of depth 64, default batch: walker-steps/s and generated states/s of
      orig_simulate (HIP-event kernel time and wall time of mc_run, median of --repeats after
      --warmup runs); the CPU yardstick (tests/native/orig_sim_host.cpp on the same walks, one
      process per 65536-walk slice, --procs at a time); the BFS yardstick (orig_generate's
      generated/s in a -workers N BFS of C2 by the same library).
  scripts/sim_bench.py --ab NAME=LIB [NAME=LIB ...] --out ...    (on an MI355X)
      the same GPU run, alternating between the product library and the experiment builds LIB
      (scripts/build_variant.sh, e.g. -DRMC_SIM_SELECT=0), one child process per run.
  scripts/sim_bench.py --resources --out profiles/sim_resources.json      (no GPU needed)
      the compiler's resource report of orig_simulate (VGPRs, spills, occupancy) for the shapes
      (3,2,3,2,5) and (5,2,2,4,6), every selection design (RMC_SIM_SELECT).
"""
import argparse
import importlib
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raft-tla_amd", "csrc")
TLA = os.path.join(ROOT, "configs", "raft_original_mc.tla")
C2 = os.path.join(ROOT, "configs", "c2.cfg")
BUILD = os.path.join(ROOT, "scripts", "_build")
C2_SHAPE = (3, 2, 3, 2, 5)


def gpu_runs(walks, depth, seed, warmup, repeats):
    """orig_simulate on c2.cfg: per-run kernel and wall seconds, and the (identical) counts."""
    sys.path.insert(0, ROOT)
    mod = importlib.import_module("raft-tla_amd")
    runs, counts = [], None
    with mod.ModelChecker(TLA, C2, seed=seed, max_depth=depth, fp_table_bytes=1 << 26, state_store_bytes=1 << 28) as mc:
        for k in range(warmup + repeats):
            t0 = time.perf_counter()
            r = mc.simulate(walks)
            wall = time.perf_counter() - t0
            c = {"verdict": r.verdict, "walks": r.walks, "steps": r.steps, "generated": r.generated, "launches": r.n_launches}
            assert counts is None or c == counts, (c, counts)
            counts = c
            if k >= warmup:
                runs.append({"kernel_s": r.kernel_seconds, "wall_s": wall})
    return runs, counts


def rates(runs, counts):
    ks = statistics.median(x["kernel_s"] for x in runs)
    ws = statistics.median(x["wall_s"] for x in runs)
    return {"kernel_s_median": ks, "kernel_s_min": min(x["kernel_s"] for x in runs), "kernel_s_max": max(x["kernel_s"] for x in runs),
            "wall_s_median": ws, "walker_steps_per_s_kernel": counts["steps"] / ks, "generated_per_s_kernel": counts["generated"] / ks,
            "walker_steps_per_s_wall": counts["steps"] / ws, "generated_per_s_wall": counts["generated"] / ws, "repeats": len(runs)}


def build_host():
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, "orig_sim_host_%d%d%d%d%d" % C2_SHAPE)
    src = [os.path.join(ROOT, "tests", "native", "orig_sim_host.cpp"), os.path.join(CSRC, "model.cpp"), os.path.join(CSRC, "orig_model.cpp")]
    if not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in src + [os.path.join(CSRC, "sim_rng.h"), os.path.join(CSRC, "orig_spec.h")]):
        defs = ["-DSHAPE_%s=%d" % (n, v) for n, v in zip(("N", "NV", "MT", "ML", "MK"), C2_SHAPE)]
        subprocess.run(["g++", "-O2", "-std=c++17", *defs, "-o", out, *src], check=True)
    return out


def cpu_yardstick(walks, depth, seed, procs, slice_walks=65536):
    """The host mirror over the same walks: one single-threaded process per slice, `procs` at a time."""
    exe = build_host()
    slices = [(w0, min(walks, w0 + slice_walks)) for w0 in range(0, walks, slice_walks)]
    t0 = time.perf_counter()
    pending, running, outs = list(slices), [], []
    while pending or running:
        while pending and len(running) < procs:
            w0, w1 = pending.pop(0)
            running.append(subprocess.Popen([exe, C2, str(seed), str(w1), str(depth), str(slice_walks), "--first", str(w0)],
                                            stdout=subprocess.PIPE, text=True))
        p = running.pop(0)
        out, _ = p.communicate()
        assert p.returncode == 0
        outs.append(json.loads(out.strip().splitlines()[-1]))
    wall = time.perf_counter() - t0
    tot = {k: sum(o[k] for o in outs) for k in ("walks", "steps", "generated")}
    assert all(o["event"] is None for o in outs)
    return {"processes": len(slices), "at_a_time": procs, "wall_s": wall, **tot,
            "walker_steps_per_s": tot["steps"] / wall, "generated_per_s": tot["generated"] / wall}


def bfs_yardstick():
    """orig_generate's generated/s in a -workers N BFS of C2 (the library's default tables)."""
    sys.path.insert(0, ROOT)
    mod = importlib.import_module("raft-tla_amd")
    best = None
    with mod.ModelChecker(TLA, C2, workers=0, seed=0x5EED) as mc:
        for _ in range(3):
            r = mc.run()
            ms = r.kernels["orig_generate"]["ms"]
            if best is None or ms < best["orig_generate_ms"]:
                best = {"generated": r.generated, "distinct": r.distinct, "orig_generate_ms": ms, "run_s": r.seconds,
                        "generated_per_s_orig_generate": r.generated / (ms * 1e-3), "generated_per_s_run": r.generated / r.seconds}
    return best


RES_TU = """#include <hip/hip_runtime.h>
#include <vector>
#include "orig_spec.h"
#include "sim_rng.h"
namespace rmc {
constexpr int BS = 256;
enum { EV_NEXT_ERROR = 0, EV_DEADLOCK = 1, EV_INV_ERROR = 2, EV_VIOLATION = 3 };
#include "orig_sim.hip"
template __global__ void orig_simulate<Orig<3, 2, 3, 2, 5>>(SimArgs);
template __global__ void orig_simulate<Orig<5, 2, 2, 4, 6>>(SimArgs);
}
"""


def resources():
    """orig_simulate alone (the product's text, the product's flags) through the compiler's resource report."""
    os.makedirs(BUILD, exist_ok=True)
    tu = os.path.join(BUILD, "sim_resources.hip")
    with open(tu, "w") as f:
        f.write(RES_TU)
    out = {}
    for sel, name in ((2, "keep_index_lane_apply"), (1, "keep_index_second_pass"), (0, "keep_work")):
        p = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950", "-munsafe-fp-atomics",
                            "-DRMC_SIM_SELECT=%d" % sel, "-I" + CSRC, "-c", tu, "-o", os.path.join(BUILD, "sim_resources.o"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, check=True)
        cur, shapes = None, {}
        for line in p.stderr.splitlines():
            m = re.search(r"Function Name: \S*orig_simulateINS_4OrigILi(\d)ELi(\d)ELi(\d)ELi(\d)ELi(\d)E", line)
            if m:
                cur = shapes.setdefault("(%s)" % ",".join(m.groups()), {})
                continue
            m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
            if m and cur is not None:
                cur[m.group(1).strip()] = int(m.group(2))
        out[name] = {"RMC_SIM_SELECT": sel, "shapes": shapes}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walks", type=int, default=1 << 20)
    ap.add_argument("--depth", type=int, default=64)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-bfs", action="store_true")
    ap.add_argument("--gpu-only", action="store_true", help="print the GPU runs as one JSON line (the --ab children)")
    ap.add_argument("--ab", metavar="NAME=LIB", nargs="+", default=None)
    ap.add_argument("--ab-rounds", type=int, default=3)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.resources:
        doc = {"kernel": "orig_simulate", "flags": "-O3 --offload-arch=gfx950 -munsafe-fp-atomics", "designs": resources()}
    elif a.gpu_only:
        runs, counts = gpu_runs(a.walks, a.depth, a.seed, a.warmup, a.repeats)
        print(json.dumps({"runs": runs, "counts": counts}))
        return
    elif a.ab:
        # the two libraries alternate, one child process per run of --repeats launches
        sides = {"product": None}
        for item in a.ab:
            name, lib = item.split("=", 1)
            sides[name] = os.path.abspath(lib)
        acc = {k: [] for k in sides}
        counts = {}
        for _ in range(a.ab_rounds):
            for name, lib in sides.items():
                env = dict(os.environ)
                if lib:
                    env["RAFTMC_LIB"] = lib
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--gpu-only", "--walks", str(a.walks), "--depth", str(a.depth),
                                    "--seed", str(a.seed), "--warmup", str(a.warmup), "--repeats", str(a.repeats)],
                                   capture_output=True, text=True, env=env, timeout=600)
                if p.returncode != 0:
                    raise SystemExit("child failed (%s): %s" % (name, p.stderr[-2000:]))
                d = json.loads(p.stdout.strip().splitlines()[-1])
                acc[name] += d["runs"]
                counts[name] = d["counts"]
        assert all(c == counts["product"] for c in counts.values()), counts   # the same walks either way
        doc = {"model": "c2.cfg", "walks": a.walks, "depth": a.depth, "seed": a.seed, "counts": counts["product"],
               "sides": {k: rates(v, counts[k]) for k, v in acc.items()}}
    else:
        runs, counts = gpu_runs(a.walks, a.depth, a.seed, a.warmup, a.repeats)
        doc = {"model": "c2.cfg", "walks": a.walks, "depth": a.depth, "seed": a.seed, "batch": 262144, "counts": counts,
               "gpu": rates(runs, counts)}
        if not a.no_cpu:
            doc["cpu_host_mirror"] = cpu_yardstick(a.walks, a.depth, a.seed, a.procs)
            assert (doc["cpu_host_mirror"]["steps"], doc["cpu_host_mirror"]["generated"]) == (counts["steps"], counts["generated"])
            doc["gpu_over_cpu_wall"] = doc["cpu_host_mirror"]["wall_s"] / doc["gpu"]["wall_s_median"]
        if not a.no_bfs:
            doc["bfs_orig_generate"] = bfs_yardstick()
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
