"""The level plan of the single-GPU -workers N search (csrc/chunk_plan.h) without a GPU:
tests/native/chunk_plan_check.cpp, a stand-alone program over chunk_plan.h alone, built with
AddressSanitizer and UBSan and run directly.  For levels of 1, 255, 256, 257 parents, the threshold
and its neighbours, 10 072 911 (C2's largest level) and one more than a multiple of the half buffer, at
sub-chunk sizes 0, 256, 768 and the default: the sub-chunks cover the level exactly and in order, every
count but the last is a whole number of workgroups, none exceeds the half buffer, the buffers
alternate, a level under the threshold is one chunk, and size 0 gives whole-allocation chunks."""
import os
import subprocess

from oracle_util import ROOT, native_build_dir


def build_check():
    out = os.path.join(native_build_dir(), "chunk_plan_check")
    csrc = os.path.join(ROOT, "raft-tla_amd", "csrc")
    src = os.path.join(ROOT, "tests", "native", "chunk_plan_check.cpp")
    deps = [src, os.path.join(csrc, "chunk_plan.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in deps):
        tmp = "%s.%d" % (out, os.getpid())    # build aside and rename: parallel workers never run a partial file
        subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", csrc, "-o", tmp, src], check=True)
        os.replace(tmp, out)
    return out


def test_chunk_plan_under_sanitizers():
    r = subprocess.run([build_check()], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
