"""Generate the log- and commit-safety fixture for raft_original (test infrastructure).

The reference is a second implementation: the generated front end (raft-tla_amd/_build/tlagen)
compiles the unmodified thirdparty/raft_original.tla through configs/raft_original_safety_mc.tla,
and its host BFS (tests/native/tlagen_host_bfs.cpp) runs in TLC's single-worker order.  Each model
is its configs/<name>.cfg with the INVARIANTS section replaced:

  parity_pair, pair6_nocommit, c1, safety_trio6   all eleven (ElectionSafety, LogMatching and the nine
                                                  of the wrapper; pair6_nocommit so loses NoCommit), full search
  safety_trio6_control                            safety_trio6.cfg with AllHaveCommitted_false only, --trace

The fixture records verdict / generated / distinct / depth / level sizes, and for a violation its
name and the counterexample (one line per state: traces, not state dumps).  `generated` at a
violation is TLC's: the whole successor lists of the parents up to and including the event's.
Needs the reference checkout for raft.tla.  safety_trio6 takes about 10 minutes and 20 GB, the
control about 4 minutes and 11 GB; `--only NAME` (repeatable) redoes single entries of the file.

    python tests/golden/make_orig_safety.py [--only NAME]... [REFERENCE_DIR]      (default: $RAFTMC_REFERENCE)
"""
import json
import os
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle_util import CONFIGS, GOLDEN, ORIG_MC, ROOT, run_oracle  # noqa: E402

TOOL = os.path.join(ROOT, "raft-tla_amd", "_build", "tlagen")
SAFETY_MC = os.path.join(CONFIGS, "raft_original_safety_mc.tla")
SAFETY = ["CommitWithinLog", "LeaderVotesQuorum", "CandidateTermNotInLog", "LeaderHasLatestOfTerm", "VotesGrantedInv",
          "QuorumLogInv", "MoreUpToDateCorrect", "LeaderCompleteness", "StateMachineSafety"]
ELEVEN = ["ElectionSafety", "LogMatching"] + SAFETY
CONTROL = "AllHaveCommitted_false"
# entry -> (cfg, invariants, --trace)
RUNS = {"parity_pair": ("parity_pair", ELEVEN, False), "pair6_nocommit": ("pair6_nocommit", ELEVEN, False),
        "c1": ("c1", ELEVEN, False), "safety_trio6": ("safety_trio6", ELEVEN, True),
        "safety_trio6_control": ("safety_trio6", [CONTROL], True)}
OUT = os.path.join(GOLDEN, "orig_safety.json")


def safety_cfg(name, invariants):
    """configs/<name>.cfg with its INVARIANTS section (the last one of these cfgs) replaced; a temp
    file, the caller unlinks it"""
    text = open(os.path.join(CONFIGS, name + ".cfg")).read()
    head, sep, _ = text.partition("INVARIANTS\n")
    assert sep, name
    fd, path = tempfile.mkstemp(suffix=".cfg")
    with os.fdopen(fd, "w") as f:
        f.write(head + "INVARIANTS\n" + "".join("    %s\n" % n for n in invariants))
    return path


def generated_bfs(ref, name, invariants, trace):
    cfg = safety_cfg(name, invariants)
    fd, gen = tempfile.mkstemp(suffix=".gen.h")
    os.close(fd)
    exe = gen + ".bin"
    try:
        subprocess.run([TOOL, SAFETY_MC, cfg, "-I", ref, "-o", gen], check=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-w", '-DTLG_FILE="%s"' % gen, "-o", exe,
                        os.path.join(ROOT, "tests", "native", "tlagen_host_bfs.cpp")], check=True)
        return json.loads(subprocess.run([exe, *(["--trace"] if trace else [])], capture_output=True, text=True, check=True).stdout)
    finally:
        for p in (cfg, gen, exe):
            if os.path.exists(p):
                os.unlink(p)


def left_on_queue_at_first_commit(name, r):
    """The host BFS does not print TLC's "states left on queue".  The control's stop point is the
    first commit, which is also where the CPU oracle stops on the same cfg with NoCommit (a name it
    knows, through configs/raft_original_mc.tla): same depth, generated and distinct, so the same
    parent and successor in the same FIFO order -- its left-on-queue is the control's.  About 13 minutes."""
    cfg = safety_cfg(name, ["NoCommit"])
    try:
        o = run_oracle("bfs", ORIG_MC, cfg, timeout=7200)
    finally:
        os.unlink(cfg)
    assert (o["verdict"], o["violated"]) == ("INVARIANT_VIOLATION", "NoCommit"), o
    assert (o["generated"], o["distinct"], o["depth"]) == (r["generated"], r["distinct"], r["depth"]), (o, r["generated"], r["distinct"])
    return o["left_on_queue"]


def main(ref, only):
    doc = json.load(open(OUT)) if only and os.path.exists(OUT) else {}
    for entry, (name, invariants, trace) in RUNS.items():
        if only and entry not in only:
            continue
        r = generated_bfs(ref, name, invariants, trace)
        assert r["err"] == 0 and r["verdict"] in ("OK", "INVARIANT_VIOLATION"), {k: v for k, v in r.items() if k != "trace"}
        doc[entry] = {"cfg": name, "invariants": invariants, "verdict": r["verdict"], "violated": r["violated"],
                      "generated": r["generated"], "distinct": r["distinct"], "depth": r["depth"], "levels": r["levels"]}
        if r["verdict"] != "OK":
            doc[entry]["trace"] = r["trace"]
        if entry == "safety_trio6_control":
            doc[entry]["left_on_queue"] = left_on_queue_at_first_commit(name, r)
        print(entry, r["verdict"], r["violated"], r["generated"], r["distinct"], r["depth"], flush=True)
        json.dump(doc, open(OUT, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    argv, only = sys.argv[1:], []
    while "--only" in argv:
        k = argv.index("--only")
        only.append(argv[k + 1])
        del argv[k:k + 2]
    main(argv[0] if argv else os.environ.get("RAFTMC_REFERENCE", "/root/reference"), only)
