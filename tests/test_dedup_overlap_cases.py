"""The cases and the checker of tests/native/orig_dedup_overlap_check.hip, on the CPU (--host-only makes no HIP
call): every case passes its checker on the outputs of the sequential routine that plays the kernel, has the
property it is named for, and the checker rejects each perturbation of those outputs.  This is what shows
that the GPU test (test_gpu_dedup_overlap.py) can fail."""
import pytest

from dedup_overlap_cases import OVERLAP_CASES
from seen_set_cases import run_cases

PERTURBATIONS = ["record_dropped", "record_duplicated", "insertion_counted_twice", "newrec_swapped"]


@pytest.fixture(scope="module")
def cases():
    return run_cases("orig_dedup_overlap_check", "--host-only")


def test_no_unlisted_case(cases):
    assert sorted(cases) == sorted(OVERLAP_CASES)


@pytest.mark.parametrize("name", OVERLAP_CASES)
def test_case_passes_its_checker_on_sequential_outputs(name, cases):
    assert cases[name]["ok"], cases[name]["first_mismatch"]


@pytest.mark.parametrize("name", OVERLAP_CASES)
def test_checker_rejects_perturbations(name, cases):
    rejected = cases[name]["rejected"]
    assert all(rejected.values()), rejected
    assert set(rejected) == set(PERTURBATIONS), rejected


def test_every_case_is_the_overlap_instantiation(cases):
    for c in cases.values():
        assert (c["props"]["per"], c["props"]["lds_slots"]) == (2, 4096)


@pytest.mark.parametrize("n, rounds", [(0, 1), (1, 1), (511, 1), (512, 1), (513, 2)])
def test_record_counts_sit_on_the_loop_boundary(n, rounds, cases):
    """Workgroups 0 and 2 hold n records, workgroup 1 a hundred: 512 = PER * BS is one trip of the loop, 513 two."""
    p = cases["overlap_records_%d" % n]["props"]
    assert p["records_max"] == max(n, 100) and p["records_min"] == min(n, 100)
    assert p["rounds_max"] == rounds
    assert cases["overlap_records_%d" % n]["n"] == 2 * n + 100
    assert p["present"] > 0


def test_window_case_overflows_a_wrapping_window(cases):
    c = cases["overlap_lds_window_wraps"]
    assert c["props"]["max_per_lds_home"] == 24 > 8
    assert c["props"]["home"] + 8 > c["props"]["lds_slots"]
    assert c["props"]["present"] >= 8


def test_duplicates_case(cases):
    c = cases["overlap_duplicates"]
    assert c["distinct"] == 200 and c["props"]["present"] == 100 and c["n"] > 3 * c["distinct"]


def test_cluster_case_crosses_the_tables_end(cases):
    c = cases["overlap_table_cluster_wraps"]
    assert c["props"]["wraps"] == 1 and c["distinct"] == 60
