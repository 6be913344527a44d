"""The per-kernel accounting of every raft_original and tlc_membership pipeline, number for number (MI355X).

Result.kernels (launches, algorithmic bytes, event-pair milliseconds) and n_launches are filled
by the host code that queues each pipeline stage: mc_run's level loop, the sharded step API that
shard.py drives, and the native sharded level loop.  tests/golden/orig_kernel_accounting.json
holds `launches` and `algo_bytes` of every kernel entry and `n_launches`, per rank, as the build
before the stage launchers were shared (one args builder and one launcher per stage) reported
them; with the fixed table and store sizes below the chunk size, and hence every count, is
determined.  Today's build must report the same numbers, and a positive time for every kernel
that was launched (an event pair that is never read back leaves 0).

Two numbers are not reproducible from run to run of one build, and the fixture does not hold them
as they are.  orig_route_blk drops duplicate records with a first-come filter in LDS, so how many
records a chunk routes depends on the order in which a workgroup's lanes arrive; the paths with a
route pass (the step API, the native loop at world > 1) add 16 B per routed record to
orig_route_blk and 24 B per received record plus 16 B per new state to orig_dedup_sh.  Every
routed record is received by some rank, so over all ranks
    sum(orig_dedup_sh bytes) - 1.5 * sum(orig_route_blk bytes) = 16 * (new states of the search),
which is reproducible: for a case with a route pass the fixture holds that difference
("dedup_minus_route") in place of the two byte counts (null), and everything else as reported.

The tlc_membership cases (MEMB_CASES, tests/golden/memb_kernel_accounting.json) pin the same three paths
of class MembGpu as the build before its stage launchers were shared reported them: the plain search in
both SYMMETRY modes and without the out-of-model invariant pass, a continue-mode search whose levels are
cut into chunks and whose completed levels spill, the step API and the native FIFO-ranked loop.  Those
paths keep the minimum key per fingerprint and have no first-come filter: two recordings of that build
agreed on every number, so the fixture holds all of them as reported.

RAFTMC_RECORD_KERNEL_ACCOUNTING=<path>: test_kernel_accounting_unchanged adds what this build
reports, pinned() applied, to the JSON file <path> instead of comparing (record twice, to two
paths, and keep the file only if both recordings are equal).
"""
import importlib
import json
import os

import pytest

from oracle_util import CONFIGS, GOLDEN, MEMB_MC, ORIG_MC

pytestmark = pytest.mark.gpu

SIZES = dict(fp_table_bytes=1 << 26, state_store_bytes=1 << 28)
PAIR = os.path.join(CONFIGS, "parity_pair.cfg")
C1 = os.path.join(CONFIGS, "c1.cfg")
FIXTURE = os.path.join(GOLDEN, "orig_kernel_accounting.json")
MEMB_FIXTURE = os.path.join(GOLDEN, "memb_kernel_accounting.json")
MEMB_SIZES = dict(fp_table_bytes=1 << 26, state_store_bytes=1 << 29)
MEMB_TWO = os.path.join(CONFIGS, "memb_two.cfg")
RECORD = os.environ.get("RAFTMC_RECORD_KERNEL_ACCOUNTING")


def _single(raftmc, cfg, workers):
    with raftmc.ModelChecker(ORIG_MC, cfg, workers=workers, **SIZES) as mc:
        return [mc.run()]


def _c1_pipelined(raftmc, monkeypatch):
    # sub-chunks of 256 parents: c1's levels of 507, 832, 864 and 558 states are cut in 2 to 4
    monkeypatch.setenv("RAFTMC_OVERLAP_STATES", "256")
    return _single(raftmc, C1, 0)


def _shard():
    return importlib.import_module("raft-tla_amd.shard")


CASES = {
    "single_parity_pair_workers0": lambda raftmc, mp: _single(raftmc, PAIR, 0),
    "single_parity_pair_workers1": lambda raftmc, mp: _single(raftmc, PAIR, 1),
    "single_c1_overlap256": _c1_pipelined,
    "step_api_world1_parity_pair": lambda raftmc, mp: [_shard().check_sharded(ORIG_MC, PAIR, 0, 1, **SIZES)],
    "native_loopback_world1_parity_pair": lambda raftmc, mp: _shard().check_loopback(ORIG_MC, PAIR, 1, **SIZES),
    "native_loopback_world2_parity_pair": lambda raftmc, mp: _shard().check_loopback(ORIG_MC, PAIR, 2, **SIZES),
}


def _memb_single(raftmc, **kw):
    # the model of test_membership_handle_rerun
    with raftmc.ModelChecker(MEMB_MC, MEMB_TWO, max_depth=14, deadlock=False, **dict(MEMB_SIZES, **kw)) as mc:
        return [mc.run()]


def _memb_continue_chunked(raftmc, mp):
    # test_later_chunks_and_spilled_parents' run: the store (and with it the chunk) too small for the search
    from test_gpu_continue import continue_run
    from test_gpu_membership import FIX, _spill_store
    store = _spill_store(raftmc, FIX["tlc:scen_ConcurrentLeaders"], margin=3.1)
    return [continue_run(raftmc, "scen_all_shipped", "tlc", state_store_bytes=store)]


MEMB_KW = dict(max_depth=14, deadlock=False, sym_tlc=True, **MEMB_SIZES)
MEMB_CASES = {
    "memb_single_memb_two_orbit": lambda raftmc, mp: _memb_single(raftmc, sym_tlc=False),
    "memb_single_memb_two_tlc": lambda raftmc, mp: _memb_single(raftmc, sym_tlc=True),
    "memb_single_memb_two_no_oom_pass": lambda raftmc, mp: _memb_single(raftmc, sym_tlc=True, inv_out_of_model=False),
    "memb_single_continue_chunked": _memb_continue_chunked,
    "memb_step_api_world1_memb_two": lambda raftmc, mp: [_shard().check_sharded(MEMB_MC, MEMB_TWO, 0, 1, **MEMB_KW)],
    "memb_native_loopback_world1_memb_two": lambda raftmc, mp: _shard().check_loopback(MEMB_MC, MEMB_TWO, 1, **MEMB_KW),
    "memb_native_loopback_world2_memb_two": lambda raftmc, mp: _shard().check_loopback(MEMB_MC, MEMB_TWO, 2, **MEMB_KW),
}
# how each family's searches end: raft_original's run out of states, memb_two stops at max_depth and the
# continue run at the last witness
VERDICTS = dict({name: "OK" for name in CASES}, **{name: "DEPTH_LIMIT" for name in MEMB_CASES})
VERDICTS["memb_single_continue_chunked"] = "INVARIANT_VIOLATION"
FIXTURE_OF = dict({name: FIXTURE for name in CASES}, **{name: MEMB_FIXTURE for name in MEMB_CASES})
CASES.update(MEMB_CASES)


def accounting(results, verdict="OK"):
    """one entry per rank: what the fixture pins"""
    out = []
    for r in results:
        assert r.verdict == verdict, r.error
        for name, k in r.kernels.items():
            assert k["ms"] > 0 or k["launches"] == 0, (name, k)
        out.append({"n_launches": r.n_launches,
                    "kernels": {name: {"launches": k["launches"], "algo_bytes": k["algo_bytes"]} for name, k in r.kernels.items()}})
    return out


def pinned(ranks):
    """what the fixture holds of one case (the module's docstring)"""
    out = {"ranks": ranks}
    if any(r["kernels"].get("orig_route_blk", {}).get("launches") for r in ranks):
        out["dedup_minus_route"] = sum(r["kernels"]["orig_dedup_sh"]["algo_bytes"] - 1.5 * r["kernels"]["orig_route_blk"]["algo_bytes"]
                                       for r in ranks)
        for r in ranks:
            r["kernels"]["orig_dedup_sh"]["algo_bytes"] = r["kernels"]["orig_route_blk"]["algo_bytes"] = None
    return out


def test_fixture_covers_every_case():
    for path in (FIXTURE, MEMB_FIXTURE):
        assert sorted(json.load(open(path))) == sorted(name for name in CASES if FIXTURE_OF[name] == path)


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_accounting_unchanged(raftmc, monkeypatch, name):
    got = accounting(CASES[name](raftmc, monkeypatch), VERDICTS[name])
    print(name, json.dumps(got))
    got = pinned(got)
    if RECORD:
        rec = json.load(open(RECORD)) if os.path.exists(RECORD) else {}
        rec[name] = got
        with open(RECORD, "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)
            f.write("\n")
        return
    assert got == json.load(open(FIXTURE_OF[name]))[name]
    if name == "single_c1_overlap256":   # some level was pipelined: more generate launches than levels
        assert got["ranks"][0]["kernels"]["orig_generate"]["launches"] > got["ranks"][0]["n_launches"]
    if name == "memb_single_continue_chunked":   # levels took several chunks, and the witness kernels ran
        k = got["ranks"][0]["kernels"]
        assert k["memb_expand"]["launches"] > got["ranks"][0]["n_launches"]
        assert k["memb_witness"]["launches"] > 0
