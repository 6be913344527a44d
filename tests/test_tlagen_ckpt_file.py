"""The generated path's checkpoint file (csrc/ckpt_file.h: the RAFTMCG1 header, check_gen_head,
read_gen_body) without a GPU: tests/native/tlagen_ckpt_check.cpp, a stand-alone program over
ckpt_file.h alone, built with AddressSanitizer and UBSan and run directly.  A write -> read round trip
of header, description, counters, 3 levels and the four body arrays of variable-width states (whole
and in chunks of one element); the file cut at every length; another family's magic, a wrong n_act,
desc_len 2^20 and inconsistent counts refused; bodies crafted with offs[i] >= words, parent[i] >= i
and a `total` beyond the file refused before anything is indexed; a write that cannot be made
leaves nothing at the final path."""
import os
import subprocess

from oracle_util import ROOT, native_build_dir


def build_check():
    out = os.path.join(native_build_dir(), "tlagen_ckpt_check")
    csrc = os.path.join(ROOT, "raft-tla_amd", "csrc")
    src = os.path.join(ROOT, "tests", "native", "tlagen_ckpt_check.cpp")
    deps = [src, os.path.join(csrc, "ckpt_file.h"), os.path.join(ROOT, "include", "raftmc.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in deps):
        tmp = "%s.%d" % (out, os.getpid())    # build aside and rename: parallel workers never run a partial file
        subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", csrc, "-o", tmp, src], check=True)
        os.replace(tmp, out)
    return out


def test_generated_checkpoint_file_under_sanitizers(tmp_path):
    r = subprocess.run([build_check(), str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
