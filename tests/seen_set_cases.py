"""The stand-alone seen-set check programs (tests/native/*_seen_set_check.hip, memb_device_check.hip):
where they are built, how a test runs one, and the case names each must report.

The programs are part of the product build (raft-tla_amd/Makefile, target `checks`), so that they exist
wherever the library does; a test builds them itself only when they are missing."""
import json
import os
import subprocess

from oracle_util import ROOT

CHECKS = os.path.join(ROOT, "raft-tla_amd", "_build", "checks")

_PROBE = ["one_home_8", "one_home_64", "one_home_600", "one_fp_many", "extremes", "exact_fill", "prepopulated"]
ORIG_CASES = (["probe_" + c for c in _PROBE] + ["dedup_sh_" + c for c in _PROBE] +
              ["merge_window_overflow", "merge_full_overlap", "merge_empty", "merge_uneven_waves",
               "dedup_plain_duplicates", "mark_count_scan",
               "scan_nblk_1", "scan_nblk_3", "scan_nblk_1023", "scan_nblk_1024", "scan_nblk_1025", "scan_nblk_3077",
               "migrate1_cluster", "migrate1_full", "migrate2_cluster", "migrate2_full",
               "route_world_1", "route_world_2", "route_world_3", "route_world_8"])
MEMB_CASES = ["memb_pipeline_chunk_1", "memb_pipeline_chunk_255", "memb_pipeline_chunk_257", "memb_pipeline_chunk_1000",
              "memb_scan_blocks_1", "memb_scan_blocks_256", "memb_scan_blocks_4095", "memb_scan_blocks_4096"]


def check_program(name):
    exe = os.path.join(CHECKS, name)
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "raft-tla_amd"), os.path.join("_build", "checks", name)],
                       check=True, timeout=1800)
    return exe


def run_cases(name, *args):
    """Run a check program once; {case name: its JSON line}.  A HIP failure (an "error" line, exit status
    2) or a missing line is the caller's to report: the lines that did come out are returned with it."""
    p = subprocess.run([check_program(name), *args], capture_output=True, text=True, timeout=300)
    lines = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    errors = [l["error"] for l in lines if "error" in l]
    assert not errors and p.returncode in (0, 1), (p.returncode, errors, p.stderr[-2000:])
    return {l["case"]: l for l in lines if "case" in l}
