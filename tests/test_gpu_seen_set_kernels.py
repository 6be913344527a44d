"""The seen-set and dedup kernels of both backends, each launched once on a synthetic adversarial input
and checked against a plain sequential model (tests/native/orig_seen_set_check.hip,
memb_seen_set_check.hip: one process per program, one JSON line per case), and the device-versus-host
equivalence of tlc_membership's packed spec (tests/native/memb_device_check.hip).  What the cases are
and that their checkers can fail is tested on the CPU by test_seen_set_cases.py."""
import json
import os
import subprocess

import pytest

from oracle_util import CONFIGS
from seen_set_cases import MEMB_CASES, ORIG_CASES, check_program, run_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def orig():
    return run_cases("orig_seen_set_check")


@pytest.fixture(scope="module")
def memb():
    return run_cases("memb_seen_set_check")


@pytest.mark.parametrize("name", ORIG_CASES)
def test_orig_kernel_contract(name, orig):
    assert name in orig, "case %s is missing from the program's output" % name
    assert orig[name]["ok"], orig[name]["first_mismatch"]


@pytest.mark.parametrize("name", MEMB_CASES)
def test_memb_kernel_contract(name, memb):
    assert name in memb, "case %s is missing from the program's output" % name
    assert memb[name]["ok"], memb[name]["first_mismatch"]


@pytest.mark.parametrize("sym_tlc", [False, True], ids=["orbit", "sym_tlc"])
def test_memb_device_matches_host(sym_tlc):
    """Every (state, slot) pair of the first levels of memb_two: action, packed successor, constraint and
    invariant verdicts and the symmetric fingerprint agree between device and host, and memb_expand's
    cells and fingerprints are the host's."""
    env = dict(os.environ)
    env.pop("SYM_TLC", None)
    if sym_tlc:
        env["SYM_TLC"] = "1"
    p = subprocess.run([check_program("memb_device_check"), os.path.join(CONFIGS, "memb_two.cfg"), "4"],
                       capture_output=True, text=True, timeout=300, env=env)
    lines = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    assert not [l for l in lines if "error" in l], (lines, p.stderr[-2000:])
    last = lines[-1]
    assert last["mismatches"] == 0, (lines, p.stderr[-2000:])
    assert last["pairs"] > 0
    assert p.returncode == 0
