"""orig_dedup_plain's instantiation for launches beside a generate (2 probes in flight per thread, a 4096-slot
LDS filter), launched once per case on a synthetic adversarial input and checked against a plain sequential
model (tests/native/orig_dedup_overlap_check.hip: one process, one JSON line per case).  What the cases are
and that their checker can fail is tested on the CPU by test_dedup_overlap_cases.py."""
import pytest

from dedup_overlap_cases import OVERLAP_CASES
from seen_set_cases import run_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return run_cases("orig_dedup_overlap_check")


@pytest.mark.parametrize("name", OVERLAP_CASES)
def test_overlap_kernel_contract(name, cases):
    assert name in cases, "case %s is missing from the program's output" % name
    assert cases[name]["ok"], cases[name]["first_mismatch"]
