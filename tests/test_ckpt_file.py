"""The checkpoint file framing (csrc/ckpt_file.h) without a GPU: tests/native/ckpt_file_check.cpp, a
stand-alone program over ckpt_file.h and host_store.h alone, built with AddressSanitizer and
UBSan and run directly.  For both family headers (RAFTMCK2, RAFTMCM1): a write -> read round trip of
header, description, per-action counters, 3 levels and the stored states; the file cut at every
length from 0 to size-1 ("not a checkpoint of this model" inside header + description, "truncated"
behind them); a wrong magic, desc_len 2^20, n_levels 0 and a wrong n_act refused; a write that
cannot be made leaves nothing at the final path."""
import os
import subprocess

from oracle_util import ROOT, native_build_dir


def build_check():
    out = os.path.join(native_build_dir(), "ckpt_file_check")
    csrc = os.path.join(ROOT, "raft-tla_amd", "csrc")
    src = os.path.join(ROOT, "tests", "native", "ckpt_file_check.cpp")
    deps = [src, os.path.join(csrc, "ckpt_file.h"), os.path.join(csrc, "host_store.h"), os.path.join(ROOT, "include", "raftmc.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in deps):
        tmp = "%s.%d" % (out, os.getpid())    # build aside and rename: parallel workers never run a partial file
        subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", csrc, "-o", tmp, src], check=True)
        os.replace(tmp, out)
    return out


def test_ckpt_file_framing_under_sanitizers(tmp_path):
    r = subprocess.run([build_check(), str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
