"""Generate the SYMMETRY Permutations(Server) fixture for raft_original (test infrastructure).

The reference is a second implementation: the generated front end (raft-tla_amd/_build/tlagen)
compiles the unmodified thirdparty/raft_original.tla through configs/raft_original_sym_mc.tla,
and its host BFS (tests/native/tlagen_host_bfs.cpp) applies SYMMETRY by TLC's rule (the least
permuted full state).  Each model is its configs/<name>.cfg with the line
`SYMMETRY ServerSymmetry` added; c5v2 runs with --max-depth 9.  The fixture records generated /
distinct / depth / level sizes.  Needs the reference checkout for raft.tla (about 35 s in all).

    python tests/golden/make_orig_symmetry.py [REFERENCE_DIR]      (default: $RAFTMC_REFERENCE, as csrc/tlagen/prebuild.py)
"""
import json
import os
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle_util import CONFIGS, GOLDEN, ROOT, cfg_variant  # noqa: E402

TOOL = os.path.join(ROOT, "raft-tla_amd", "_build", "tlagen")
SYM_MC = os.path.join(CONFIGS, "raft_original_sym_mc.tla")
MODELS = [("parity_pair", 0), ("parity_trio", 0), ("c1", 0), ("c5v2", 9)]
OUT = os.path.join(GOLDEN, "orig_symmetry.json")


def generated_bfs(ref, name, max_depth):
    cfg = cfg_variant(os.path.join(CONFIGS, name + ".cfg"), append="SYMMETRY ServerSymmetry\n")
    fd, gen = tempfile.mkstemp(suffix=".gen.h")
    os.close(fd)
    exe = gen + ".bin"
    try:
        subprocess.run([TOOL, SYM_MC, cfg, "-I", ref, "-o", gen], check=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-w", '-DTLG_FILE="%s"' % gen, "-o", exe,
                        os.path.join(ROOT, "tests", "native", "tlagen_host_bfs.cpp")], check=True)
        args = ["--max-depth", str(max_depth)] if max_depth else []
        return json.loads(subprocess.run([exe, *args], capture_output=True, text=True, check=True).stdout)
    finally:
        for p in (cfg, gen, exe):
            if os.path.exists(p):
                os.unlink(p)


def main(ref):
    doc = {}
    for name, max_depth in MODELS:
        r = generated_bfs(ref, name, max_depth)
        assert r["err"] == 0 and r["verdict"] == ("DEPTH_LIMIT" if max_depth else "OK"), r
        doc[name] = {"generated": r["generated"], "distinct": r["distinct"], "depth": r["depth"], "levels": r["levels"],
                     "max_depth": max_depth, "verdict": r["verdict"]}
        print(name, doc[name]["generated"], doc[name]["distinct"], doc[name]["depth"], flush=True)
    json.dump(doc, open(OUT, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("RAFTMC_REFERENCE", "/root/reference"))
