"""The level plan behind a level hoist (csrc/chunk_plan.h) without a GPU:
tests/native/chunk_plan_hoist_check.cpp, a stand-alone program over chunk_plan.h alone, built with
AddressSanitizer and UBSan and run directly.  Levels of 1, 255, 256, 257, sub - 1, sub, sub + 1, 2 sub,
2 sub + 1 and 5 sub + 17 parents, with the first 0, 256, sub and half_cap of them generated ahead into
either half: the chunks cover the level once and in order, chunk 0 is the prefix in its buffer,
neighbours alternate buffers, every chunk but the last is whole workgroups and at most a half, with no
prefix the plan is today's element for element, and a prefix the level cannot have had gives no plan."""
import os
import subprocess

from oracle_util import ROOT, native_build_dir


def build_check():
    out = os.path.join(native_build_dir(), "chunk_plan_hoist_check")
    csrc = os.path.join(ROOT, "raft-tla_amd", "csrc")
    src = os.path.join(ROOT, "tests", "native", "chunk_plan_hoist_check.cpp")
    deps = [src, os.path.join(csrc, "chunk_plan.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in deps):
        tmp = "%s.%d" % (out, os.getpid())    # build aside and rename: parallel workers never run a partial file
        subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", csrc, "-o", tmp, src], check=True)
        os.replace(tmp, out)
    return out


def test_chunk_plan_hoist_under_sanitizers():
    r = subprocess.run([build_check()], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
