"""Generate the action-property fixture for raft_original (test infrastructure).

The reference is tests/native/orig_actions_host.cpp `bfs`: a single-worker FIFO BFS with
tests/native/orig_host_bfs.cpp's contract (TLC's order and stop point over the product's packed successor
function) that checks the cfg's PROPERTIES with a literal evaluator of each definition -- sequences element
by element, Restart(i) conjunct by conjunct -- not with the packed code the kernels compile.  Entries:

  pair7                        configs/pair7.cfg, no properties; the CPU oracle's bfs of the same cfg is run
                               here once and must report the same counts (this pins the new shape)
  pair7_commit_regress         configs/pair7_commit_regress.cfg, MC_COMPAT_INV_OUT_OF_MODEL set
  pair7_commit_regress_inmodel the same with the flag cleared
  parity_pair_stepdown         configs/parity_pair_stepdown.cfg (the control)
  parity_pair_actions, c1_actions, pair6_actions, safety_trio6_actions
                               the four holding properties (safety_trio6: about 70 s on one core, here only)

Each records verdict, name, stop-point counters, level sizes, per-action [generated, distinct] and, for a
violation, the counterexample (one line per state).

    python tests/golden/make_orig_actions.py [--only NAME]...
"""
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle_util import CONFIGS, GOLDEN, ORIG_MC, ROOT, native_build_dir, run_oracle  # noqa: E402

OUT = os.path.join(GOLDEN, "orig_actions.json")
# entry -> (cfg, shape, extra arguments)
RUNS = {
    "pair7": ("pair7", (2, 1, 2, 1, 7), []),
    "pair7_commit_regress": ("pair7_commit_regress", (2, 1, 2, 1, 7), []),
    "pair7_commit_regress_inmodel": ("pair7_commit_regress", (2, 1, 2, 1, 7), ["--no-inv-oom"]),
    "parity_pair_stepdown": ("parity_pair_stepdown", (2, 1, 2, 1, 5), []),
    "parity_pair_actions": ("parity_pair_actions", (2, 1, 2, 1, 5), []),
    "c1_actions": ("c1_actions", (3, 1, 2, 1, 2), []),
    "pair6_actions": ("pair6_actions", (2, 1, 2, 1, 6), []),
    "safety_trio6_actions": ("safety_trio6_actions", (3, 1, 2, 1, 6), []),
}


def build_actions_host(shape):
    """Compile tests/native/orig_actions_host.cpp for one shape (as test_sim_host builds its mirror)."""
    out = os.path.join(native_build_dir(), "orig_actions_host_%d%d%d%d%d" % shape)
    csrc = os.path.join(ROOT, "raft-tla_amd", "csrc")
    src = [os.path.join(ROOT, "tests", "native", "orig_actions_host.cpp"), os.path.join(csrc, "model.cpp"), os.path.join(csrc, "orig_model.cpp")]
    deps = src + [os.path.join(csrc, h) for h in ("orig_spec.h", "orig_text.h", "sim_rng.h", "common.h", "model.h")]
    if os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps):
        return out
    tmp = "%s.%d" % (out, os.getpid())
    subprocess.run(["g++", "-O2", "-std=c++17", "-DSHAPE_N=%d" % shape[0], "-DSHAPE_NV=%d" % shape[1], "-DSHAPE_MT=%d" % shape[2],
                    "-DSHAPE_ML=%d" % shape[3], "-DSHAPE_MK=%d" % shape[4], "-o", tmp, *src], check=True)
    os.replace(tmp, out)
    return out


def actions_host(shape, *args, timeout=600):
    """The harness's JSON line."""
    out = subprocess.run([build_actions_host(shape), *map(str, args)], capture_output=True, text=True, check=True, timeout=timeout).stdout
    return json.loads(out.strip().splitlines()[-1])


def main(only):
    doc = json.load(open(OUT)) if only and os.path.exists(OUT) else {}
    for entry, (cfg, shape, extra) in RUNS.items():
        if only and entry not in only:
            continue
        r = actions_host(shape, "bfs", os.path.join(CONFIGS, cfg + ".cfg"), *extra, timeout=3600)
        e = {"cfg": cfg, "shape": list(shape), "inv_out_of_model": "--no-inv-oom" not in extra, "verdict": r["verdict"],
             "violated": r["violated"], "generated": r["generated"], "distinct": r["distinct"], "left_on_queue": r["left_on_queue"],
             "depth": r["depth"], "levels": r["levels"], "actions": r["actions"]}
        if r["verdict"] != "OK":
            e["trace"] = [s["state"] for s in r["trace"]]
            e["trace_actions"] = [s["action"] for s in r["trace"]]
        if entry == "pair7":
            o = run_oracle("bfs", ORIG_MC, os.path.join(CONFIGS, "pair7.cfg"), timeout=7200)
            same = all(o[k] == r[k] for k in ("verdict", "generated", "distinct", "depth", "actions"))
            assert same, (o, r)
            e["oracle_agrees"] = same
        doc[entry] = e
        print(entry, e["verdict"], e["violated"], e["generated"], e["distinct"], e["depth"], flush=True)
        json.dump(doc, open(OUT, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    argv, only = sys.argv[1:], []
    while "--only" in argv:
        k = argv.index("--only")
        only.append(argv[k + 1])
        del argv[k:k + 2]
    main(only)
