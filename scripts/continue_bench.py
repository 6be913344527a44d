#!/usr/bin/env python3
"""Measurements of continue mode (bench.py is raft_original's BFS and is not involved).

  scripts/continue_bench.py --parent DIR --out profiles/continue_scenarios.json      (on an MI355X)

Per group of scenario properties (configs/scen_all_*.cfg) and SYMMETRY mode:
  * the one continue run by this tree's library: seconds_total and seconds_kernels of mc_run and the
    memb_witness share of the kernel time;
  * the sum over the group's single-property runs (configs/scen_<property>.cfg) by the PARENT
    commit's library: DIR is a checkout of the parent with its package built
    (DIR/raft-tla_amd/_build/libraftmc.so), e.g. `git worktree add DIR HEAD~1 && make -C DIR/raft-tla_amd`;
  * for the shipped group, the continue run against the parent's single scen_ConcurrentLeaders run: the
    same search to the same stop point, so the difference is the mode's overhead.
Every figure is the median of --repeats runs after --warmup runs on one handle, one child process per
(library, cfg, mode): the two trees' packages have the same module name.  The counters of every run are
compared (witness against its single-property run) before a time is reported.
"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = {
    "scen_all_shipped": ["BoundedTrace", "ConcurrentLeaders", "EntryCommitted", "FirstBecomeLeader", "FirstCommit", "FirstRestart",
                         "LeadershipChange"],
    "scen_all_dynamic3": ["AddCommits", "AddSucessful", "MembershipChange", "MembershipChangeCommits", "MultipleMembershipChanges"],
    "scen_all_grow2": ["MultipleMembershipChangesCommit", "LeaderChangesDuringConfChange"],
}
SIZES = dict(fp_table_bytes=1 << 26, state_store_bytes=1 << 29)


def worker(tree, cfg, mode, cont, warmup, repeats):
    """runs of one cfg by the package of `tree` (configs always from this tree); one JSON line"""
    sys.path.insert(0, tree)
    mod = importlib.import_module("raft-tla_amd")
    tla = os.path.join(ROOT, "configs", "raft_membership_mc.tla")
    runs, counts = [], None
    with mod.ModelChecker(tla, os.path.join(ROOT, "configs", cfg + ".cfg"), sym_tlc=mode == "tlc", deadlock=False, **SIZES) as mc:
        if cont:
            mc.set_continue()
        for k in range(warmup + repeats):
            t0 = time.perf_counter()
            r = mc.run()
            wall = time.perf_counter() - t0
            c = {"verdict": r.verdict, "violated": r.violated, "depth": r.depth, "generated": r.generated, "distinct": r.distinct,
                 "left_on_queue": r.left_on_queue}
            if cont:
                c["witnesses"] = [{"invariant": w.invariant, "depth": w.depth, "generated": w.generated, "distinct": w.distinct,
                                   "left_on_queue": w.left_on_queue} for w in r.witnesses]
            assert counts is None or c == counts, (c, counts)
            counts = c
            if k >= warmup:
                runs.append({"seconds_total": r.seconds, "seconds_kernels": r.kernel_seconds, "wall_s": wall,
                             "kernels_ms": {n: v["ms"] for n, v in r.kernels.items()}})
    print(json.dumps({"runs": runs, "counts": counts}))


def child(tree, cfg, mode, cont, a):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", tree, cfg, mode, "1" if cont else "0",
                        "--warmup", str(a.warmup), "--repeats", str(a.repeats)], capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise SystemExit("child failed (%s %s %s): %s" % (tree, cfg, mode, p.stderr[-2000:]))
    return json.loads(p.stdout.strip().splitlines()[-1])


def med(runs, key):
    return statistics.median(x[key] for x in runs)


def summary(d):
    ks = {n: statistics.median(x["kernels_ms"][n] for x in d["runs"]) for n in d["runs"][0]["kernels_ms"]}
    return {"seconds_total": med(d["runs"], "seconds_total"), "seconds_kernels": med(d["runs"], "seconds_kernels"),
            "wall_s": med(d["runs"], "wall_s"), "kernels_ms": ks, "repeats": len(d["runs"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="checkout of the parent commit with raft-tla_amd/_build/libraftmc.so built")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--groups", nargs="+", default=sorted(GROUPS))
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", nargs=4, metavar=("TREE", "CFG", "MODE", "CONTINUE"))
    a = ap.parse_args()
    if a.worker:
        worker(a.worker[0], a.worker[1], a.worker[2], a.worker[3] == "1", a.warmup, a.repeats)
        return
    if not a.parent or not os.path.exists(os.path.join(a.parent, "raft-tla_amd", "_build", "libraftmc.so")):
        raise SystemExit("--parent DIR: a checkout of the parent commit with its library built")
    parent = os.path.abspath(a.parent)
    doc = {"sizes": SIZES, "warmup": a.warmup, "repeats": a.repeats, "groups": {}}
    for cfg in a.groups:
        for mode in ("orbit", "tlc"):
            c = child(ROOT, cfg, mode, True, a)
            cs = summary(c)
            wit = {w["invariant"]: w for w in c["counts"]["witnesses"]}
            assert sorted(wit) == sorted(GROUPS[cfg]), c["counts"]
            singles = {}
            for prop in GROUPS[cfg]:
                s = child(parent, "scen_" + prop, mode, False, a)
                k = s["counts"]
                assert k["violated"] == prop and all(k[f] == wit[prop][f] for f in ("depth", "generated", "distinct", "left_on_queue")), (k, wit[prop])
                singles[prop] = summary(s)
            entry = {
                "continue": cs,
                "witness_share_of_kernel_time": cs["kernels_ms"]["memb_witness"] / sum(cs["kernels_ms"].values()),
                "parent_single_runs": singles,
                "parent_single_runs_sum": {f: sum(v[f] for v in singles.values()) for f in ("seconds_total", "seconds_kernels", "wall_s")},
                "witnesses": c["counts"]["witnesses"],
            }
            entry["continue_over_parent_sum_seconds_total"] = cs["seconds_total"] / entry["parent_single_runs_sum"]["seconds_total"]
            deepest = max(GROUPS[cfg], key=lambda p: (wit[p]["depth"], wit[p]["generated"]))
            # the same search to the same stop point: the mode's overhead
            entry["against_deepest_single"] = {
                "property": deepest,
                "continue_seconds_total": cs["seconds_total"], "parent_seconds_total": singles[deepest]["seconds_total"],
                "continue_seconds_kernels": cs["seconds_kernels"], "parent_seconds_kernels": singles[deepest]["seconds_kernels"]}
            doc["groups"]["%s/%s" % (cfg, mode)] = entry
            print(cfg, mode, "continue %.4f s, parent singles sum %.4f s, deepest single (%s) %.4f s, witness share %.3f" % (
                cs["seconds_total"], entry["parent_single_runs_sum"]["seconds_total"], deepest, singles[deepest]["seconds_total"],
                entry["witness_share_of_kernel_time"]), flush=True)
    text = json.dumps(doc, indent=1, sort_keys=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
