"""The seen-set check programs' own cases and checkers, on the CPU (--host-only makes no HIP call):
every case passes its checker on the outputs of a sequential host routine that plays the kernel, every
case has the property it is named for, and the checker rejects each perturbation of those outputs.
This is what shows that the GPU test (test_gpu_seen_set_kernels.py) can fail."""
import pytest

from seen_set_cases import MEMB_CASES, ORIG_CASES, run_cases

PERTURBATIONS = ["record_dropped", "record_duplicated", "key_raised", "insertion_counted_twice", "newrec_swapped",
                 "woff_off_by_one"]

# the perturbations each case must have been put through (a case with nothing to perturb, such as the
# empty region, has none; the full-table cases are checked by their error flag alone)
_TABLE = ["record_dropped", "record_duplicated", "insertion_counted_twice"]
_SCAN = ["woff_off_by_one", "insertion_counted_twice"]
REJECTS = {}
for _c in ORIG_CASES:
    if _c.startswith("probe_"):
        REJECTS[_c] = _TABLE + ["key_raised"]
    elif _c.startswith("dedup_sh_") or _c.startswith("route_") or _c == "migrate1_cluster":
        REJECTS[_c] = _TABLE
    elif _c.startswith("scan_nblk_"):
        REJECTS[_c] = _SCAN
for _c in ("probe_exact_fill", "dedup_sh_exact_fill"):          # no empty slot to put a duplicate in
    REJECTS[_c] = [p for p in REJECTS[_c] if p != "record_duplicated"]
REJECTS["migrate2_cluster"] = _TABLE + ["key_raised"]
REJECTS["merge_window_overflow"] = REJECTS["merge_uneven_waves"] = ["record_dropped", "record_duplicated", "key_raised"]
REJECTS["merge_full_overlap"] = ["record_dropped", "key_raised"]
REJECTS["dedup_plain_duplicates"] = ["record_dropped", "record_duplicated", "insertion_counted_twice", "newrec_swapped"]
REJECTS["mark_count_scan"] = ["record_dropped", "insertion_counted_twice", "woff_off_by_one"]
for _c in MEMB_CASES:
    REJECTS[_c] = _SCAN if _c.startswith("memb_scan_blocks_") else PERTURBATIONS


@pytest.fixture(scope="module")
def orig():
    return run_cases("orig_seen_set_check", "--host-only")


@pytest.fixture(scope="module")
def memb():
    return run_cases("memb_seen_set_check", "--host-only")


def _case(name, orig, memb):
    got = memb if name.startswith("memb_") else orig
    assert name in got, "case %s is missing from the program's output" % name
    return got[name]


def test_no_unlisted_case(orig, memb):
    assert sorted(orig) == sorted(ORIG_CASES)
    assert sorted(memb) == sorted(MEMB_CASES)


@pytest.mark.parametrize("name", ORIG_CASES + MEMB_CASES)
def test_case_passes_its_checker_on_sequential_outputs(name, orig, memb):
    c = _case(name, orig, memb)
    assert c["ok"], c["first_mismatch"]


@pytest.mark.parametrize("name", ORIG_CASES + MEMB_CASES)
def test_checker_rejects_perturbations(name, orig, memb):
    c = _case(name, orig, memb)
    assert all(c["rejected"].values()), c["rejected"]
    assert set(REJECTS.get(name, [])) <= set(c["rejected"]), (name, c["rejected"])


def test_every_perturbation_is_exercised(orig, memb):
    seen = set()
    for c in list(orig.values()) + list(memb.values()):
        seen |= set(c["rejected"])
    assert seen == set(PERTURBATIONS)


@pytest.mark.parametrize("name", ["probe_one_home_8", "probe_one_home_64", "probe_one_home_600", "dedup_sh_one_home_8",
                                  "dedup_sh_one_home_64", "dedup_sh_one_home_600", "memb_pipeline_chunk_255",
                                  "memb_pipeline_chunk_257", "memb_pipeline_chunk_1000"])
def test_wrap_cases_cross_the_last_slot(name, orig, memb):
    assert _case(name, orig, memb)["props"]["wraps"] == 1


@pytest.mark.parametrize("name", ["migrate1_cluster", "migrate2_cluster"])
def test_migrate_source_cluster_crosses_the_end(name, orig, memb):
    assert _case(name, orig, memb)["props"]["src_wraps"] == 1


@pytest.mark.parametrize("name", ["merge_window_overflow", "merge_full_overlap", "dedup_plain_duplicates"])
def test_window_cases_overflow_the_lds_window(name, orig, memb):
    assert _case(name, orig, memb)["props"]["max_per_lds_home"] > 8


def test_overlap_case_overlaps(orig, memb):
    c = _case("merge_full_overlap", orig, memb)
    p = c["props"]
    assert c["n"] == p["region"] == c["distinct"]
    assert p["total"] + 2 * p["nov"] > p["region"]


@pytest.mark.parametrize("name", ["probe_exact_fill", "dedup_sh_exact_fill"])
def test_exact_fill_fills_exactly(name, orig, memb):
    c = _case(name, orig, memb)
    assert c["distinct"] == c["props"]["slots"]


def test_scan_cases_cover_fewer_and_several_blocks_per_thread(orig, memb):
    per = {n: _case("scan_nblk_%d" % n, orig, memb)["props"]["per_thread"] for n in (1, 3, 1023, 1024, 1025, 3077)}
    assert per == {1: 1, 3: 1, 1023: 1, 1024: 1, 1025: 2, 3077: 4}
