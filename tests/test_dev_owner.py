"""The owner of a backend's device allocations, events and streams (csrc/dev_owner.h) without a GPU:
tests/native/dev_owner_check.cpp, a stand-alone program over dev_owner.h alone with a counting
stand-in for the runtime, built with AddressSanitizer and UBSan and run directly.  A creation that
fails after k of n releases exactly those k, once, and leaves an owner that allocates again;
release() twice is clean; a stream is destroyed after everything else; a handle is freed and
re-created in place; a moved-from owner is empty."""
import os
import subprocess

from oracle_util import ROOT, native_build_dir


def build_check():
    out = os.path.join(native_build_dir(), "dev_owner_check")
    csrc = os.path.join(ROOT, "raft-tla_amd", "csrc")
    src = os.path.join(ROOT, "tests", "native", "dev_owner_check.cpp")
    deps = [src, os.path.join(csrc, "dev_owner.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in deps):
        tmp = "%s.%d" % (out, os.getpid())    # build aside and rename: parallel workers never run a partial file
        subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", csrc, "-o", tmp, src], check=True)
        os.replace(tmp, out)
    return out


def test_dev_owner_under_sanitizers():
    r = subprocess.run([build_check()], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
