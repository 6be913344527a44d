"""The per-kernel accounting of every raft_original pipeline, number for number (MI355X).

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

RAFTMC_RECORD_KERNEL_ACCOUNTING=<path>: test_kernel_accounting_unchanged adds what this build
reports, pinned() applied, to the JSON file <path> instead of comparing (record twice, to two
paths, and keep the file only if both recordings are equal).
"""
import importlib
import json
import os

import pytest

from oracle_util import CONFIGS, GOLDEN, ORIG_MC

pytestmark = pytest.mark.gpu

SIZES = dict(fp_table_bytes=1 << 26, state_store_bytes=1 << 28)
PAIR = os.path.join(CONFIGS, "parity_pair.cfg")
C1 = os.path.join(CONFIGS, "c1.cfg")
FIXTURE = os.path.join(GOLDEN, "orig_kernel_accounting.json")
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


def accounting(results):
    """one entry per rank: what the fixture pins"""
    out = []
    for r in results:
        assert r.verdict == "OK", r.error
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
    assert sorted(json.load(open(FIXTURE))) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_accounting_unchanged(raftmc, monkeypatch, name):
    got = accounting(CASES[name](raftmc, monkeypatch))
    print(name, json.dumps(got))
    got = pinned(got)
    if RECORD:
        rec = json.load(open(RECORD)) if os.path.exists(RECORD) else {}
        rec[name] = got
        with open(RECORD, "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)
            f.write("\n")
        return
    assert got == json.load(open(FIXTURE))[name]
    if name == "single_c1_overlap256":   # some level was pipelined: more generate launches than levels
        assert got["ranks"][0]["kernels"]["orig_generate"]["launches"] > got["ranks"][0]["n_launches"]
