"""Time a recovery on the generated path: full-size C2 (raft_original.tla through the SANY-subset front
end, prebuilt source, workers=0) checkpointed at depth D and recovered with max_depth = D, so only
the load (file -> host -> device) and the seen-set rebuild (tlg_rebuild_k) run.

    python scripts/tlagen_recover_time.py [--depth D] [--reps N] [--dir DIR] [--source X.gen.hip] [--init-only]

D defaults to 11: 1,453,017 stored states, the deepest C2 checkpoint under about 4 GiB.  DIR (the
checkpoint's directory) should be on local disk; the default is the system's temporary directory.
Every figure is the median of N runs (default 5) on a warm handle -- one untimed run first, which
allocates the device buffers and loads the code object; the page cache holds the file after it, so
the load figure is file -> host -> device without the disk.  Beside them: the search from Init to
depth D on the same handle sizes.  --init-only prints that last figure alone: it is how the same
search is timed on another build of the library (RAFTMC_LIB, with --source naming that build's
generated source), which knows no checkpoints."""
import argparse
import importlib
import json
import os
import re
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--depth", type=int, default=11)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--dir", default=tempfile.gettempdir())
ap.add_argument("--source", default=os.path.join(ROOT, "raft-tla_amd", "_build", "tlagen_co", "c2.gen.hip"))
ap.add_argument("--init-only", action="store_true")
args = ap.parse_args()

rm = importlib.import_module("raft-tla_amd")
CFG = os.path.join(ROOT, "configs", "c2.cfg")
SIZES = dict(fp_table_bytes=1 << 28, state_store_bytes=16 << 30)
D = args.depth


def open_c2():
    return rm.ModelChecker(args.source, CFG, frontend="generated", workers=0, max_depth=D, **SIZES)


def median(xs):
    return statistics.median(xs)


def run_with_stderr(mc):
    """mc.run() with the library's RAFTMC_TLAGEN_TIMING lines (stderr of this process) captured"""
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as f:
        os.dup2(f.fileno(), 2)
        try:
            r = mc.run()
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        f.seek(0)
        return r, f.read().decode(errors="replace")


def from_init():
    with open_c2() as mc:
        mc.run()   # warm-up: allocation, code object
        runs = []
        for _ in range(args.reps):
            r = mc.run()
            assert r.verdict == "DEPTH_LIMIT" and r.depth == D, (r.verdict, r.error)
            runs.append((r.seconds, r.kernel_seconds))
    return dict(what="C2 from Init to depth %d, generated path, workers=0" % D, library=os.environ.get("RAFTMC_LIB") or "this build",
                distinct=r.distinct, generated=r.generated, reps=args.reps,
                run_s_median=round(median([x[0] for x in runs]), 4), kernel_s_median=round(median([x[1] for x in runs]), 4),
                run_s_all=[round(x[0], 4) for x in runs])


if args.init_only:
    print(json.dumps(from_init()), flush=True)
    sys.exit(0)

path = os.path.join(args.dir, "tlagen_recover_time.%d.ckpt" % os.getpid())
try:
    with open_c2() as mc:
        mc.set_checkpoint(path, D)   # every D levels: the one file, at depth D
        w = mc.run()
    assert w.verdict == "DEPTH_LIMIT" and os.path.exists(path), (w.verdict, w.error)
    size = os.path.getsize(path)
    print(json.dumps(dict(what="checkpoint written at depth %d" % D, file_bytes=size, file_gib=round(size / 2 ** 30, 3), states=w.distinct,
                          writer_run_s=round(w.seconds, 3), writer_kernel_s=round(w.kernel_seconds, 3))), flush=True)
    os.environ["RAFTMC_TLAGEN_TIMING"] = "1"
    with open_c2() as mc:
        mc.set_recover(path)
        mc.run()   # warm-up
        runs = []
        for _ in range(args.reps):
            r, err = run_with_stderr(mc)
            assert (r.verdict, r.distinct, r.generated, r.depth) == ("DEPTH_LIMIT", w.distinct, w.generated, D), (r.verdict, r.error)
            m = re.search(r"recover read \+ upload ([0-9.]+) s", err)
            runs.append((float(m.group(1)), r.kernel_seconds * 1e3, r.seconds))
    del os.environ["RAFTMC_TLAGEN_TIMING"]
    load_s, rebuild_ms, run_s = (median([x[k] for x in runs]) for k in range(3))
    print(json.dumps(dict(what="recover with max_depth = %d: load and rebuild only" % D, reps=args.reps, load_s_median=round(load_s, 4),
                          load_gib_per_s=round(size / 2 ** 30 / load_s, 2), rebuild_kernel_ms_median=round(rebuild_ms, 3),
                          rebuild_states_per_s=round(w.distinct / (rebuild_ms / 1e3)), mc_run_s_median=round(run_s, 4),
                          all=[[round(a, 4), round(b, 3), round(c, 4)] for a, b, c in runs])), flush=True)
    print(json.dumps(from_init()), flush=True)
finally:
    for p in (path, path + ".tmp"):
        if os.path.exists(p):
            os.remove(p)
