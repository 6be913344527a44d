"""The multi-GPU checkpoint files (csrc/ckpt_file.h: the manifest, the rank files and ckpt::open_source,
which every recovery at another GPU count reads through) without a GPU: tests/native/
shard_ckpt_check.cpp, a stand-alone program over ckpt_file.h alone, built with AddressSanitizer and
UBSan and run directly.  A write -> read round trip of the manifest and three rank files; the manifest
and a rank file cut at every length ("not a checkpoint of this model" inside header + description,
"truncated" behind them, never a read past the end); a wrong world, generation, rank, seed or model;
a missing rank file; level tables that disagree with the manifest; the rank files a new manifest
makes stale; a single-GPU file of either search order as a source of one part."""
import os
import subprocess

from oracle_util import ROOT, native_build_dir


def build_check():
    out = os.path.join(native_build_dir(), "shard_ckpt_check")
    csrc = os.path.join(ROOT, "raft-tla_amd", "csrc")
    src = os.path.join(ROOT, "tests", "native", "shard_ckpt_check.cpp")
    deps = [src, os.path.join(csrc, "ckpt_file.h"), os.path.join(ROOT, "include", "raftmc.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in deps):
        tmp = "%s.%d" % (out, os.getpid())    # build aside and rename: parallel workers never run a partial file
        subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", csrc, "-o", tmp, src], check=True)
        os.replace(tmp, out)
    return out


def test_shard_ckpt_files_under_sanitizers(tmp_path):
    r = subprocess.run([build_check(), str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
