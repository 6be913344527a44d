"""SYMMETRY Permutations(Server) for raft_original on the GPU (configs/raft_original_sym_mc.tla +
`SYMMETRY ServerSymmetry`): one seen-set entry per orbit (orig_generate_sym, S::fp_sym), the kept
state the successor as generated.  The reference is tests/golden/orig_symmetry.json (the generated
front end's host BFS with TLC's rule); the single-worker per-action counts are those of the host
mirror tests/native/orig_sym_host.cpp over the same header."""
import json
import os

import pytest

from oracle_util import CONFIGS, GOLDEN, ORIG_MC, run_oracle
from test_orig_symmetry_host import SYM_MC, sym_cfg, sym_host
from test_sim_host import pair_noleader_cfg

pytestmark = pytest.mark.gpu

SMALL = dict(fp_table_bytes=1 << 26, state_store_bytes=1 << 28)
FIXTURE = json.load(open(os.path.join(GOLDEN, "orig_symmetry.json")))


@pytest.fixture(scope="module")
def cfgs():
    """name -> its cfg with the SYMMETRY line (temp files, removed at the end of the module)."""
    paths = {n: sym_cfg(n) for n in FIXTURE}
    yield paths
    for p in paths.values():
        os.unlink(p)


@pytest.fixture(scope="module")
def mirror():
    """name -> the host mirror's run, computed once per model"""
    cache = {}

    def get(name):
        if name not in cache:
            g = FIXTURE[name]
            cache[name] = sym_host(name, *(["--max-depth", g["max_depth"]] if g["max_depth"] else []))
        return cache[name]
    return get


@pytest.mark.parametrize("workers", [1, 0])
@pytest.mark.parametrize("name", sorted(FIXTURE))
def test_counts_equal_the_fixture(raftmc, cfgs, mirror, name, workers):
    g = FIXTURE[name]
    r = raftmc.check(SYM_MC, cfgs[name], workers=workers, max_depth=g["max_depth"], **SMALL)
    assert r.verdict == g["verdict"], r.error
    assert (r.generated, r.distinct, r.depth) == (g["generated"], g["distinct"], g["depth"])
    assert [lv[0] for lv in r.levels] == g["levels"]
    assert sum(v[0] for v in r.actions.values()) == g["generated"] - 1   # Init is generated, by no action
    if workers == 1:   # TLC's single-worker FIFO first-found order over orbits
        assert r.actions == mirror(name)["actions"]
    else:
        assert {k: v[0] for k, v in r.actions.items()} == {k: v[0] for k, v in mirror(name)["actions"].items()}
        assert sum(v[1] for v in r.actions.values()) == g["distinct"] - 1


def trace_states(r):
    return [" ".join(blk.split("\n")[1:]) for blk in r.trace_text.strip().split("\n\n")]


def test_noleader_counterexample_under_symmetry(raftmc, tmp_path):
    """parity_pair + NoLeader: the counterexample is as long as the unsymmetric search's, and since the
    kept states are successors as generated, it is a behaviour of the model without SYMMETRY."""
    plain = pair_noleader_cfg()
    sym = tmp_path / "pair_noleader_sym.cfg"
    sym.write_text(open(plain).read() + "\nSYMMETRY ServerSymmetry\n")
    try:
        a = raftmc.check(ORIG_MC, plain, **SMALL)
        for workers in (1, 0):
            b = raftmc.check(SYM_MC, str(sym), workers=workers, **SMALL)
            assert (b.verdict, b.violated, b.exit_code) == ("INVARIANT_VIOLATION", "NoLeader", 12), b.error
            assert b.depth == a.depth and len(trace_states(b)) == len(trace_states(a))
            assert b.distinct < a.distinct
            p = tmp_path / ("trace%d.txt" % workers)
            p.write_text("\n".join(trace_states(b)) + "\n")
            o = run_oracle("check-trace", ORIG_MC, plain, "--golden", str(p))
            assert o["valid"] and o["violated"] == "NoLeader" and o["length"] == len(trace_states(b)), o
    finally:
        os.unlink(plain)


@pytest.mark.parametrize("workers", [1, 0])
def test_checkpoint_recover(raftmc, cfgs, tmp_path, workers):
    """parity_trio under SYMMETRY stopped at level 6 with a checkpoint per level resumes (also on a
    larger seen-set) to the uninterrupted counts; the checkpoint's description records the symmetry,
    so it does not resume an unsymmetric search, nor the reverse."""
    g = FIXTURE["parity_trio"]
    ck, ck_plain = str(tmp_path / "sym.ckpt"), str(tmp_path / "plain.ckpt")
    plain = os.path.join(CONFIGS, "parity_trio.cfg")
    with raftmc.ModelChecker(SYM_MC, cfgs["parity_trio"], max_depth=6, workers=workers, **SMALL) as mc:
        mc.set_checkpoint(ck, 1)
        a = mc.run()
    assert a.verdict == "DEPTH_LIMIT" and a.depth == 6 and os.path.exists(ck)
    assert [lv[0] for lv in a.levels] == g["levels"][:6]
    for table in (1 << 26, 1 << 28):
        with raftmc.ModelChecker(SYM_MC, cfgs["parity_trio"], workers=workers, fp_table_bytes=table, state_store_bytes=1 << 28) as mc:
            mc.set_recover(ck)
            b = mc.run()
        assert (b.verdict, b.generated, b.distinct, b.depth) == ("OK", g["generated"], g["distinct"], g["depth"]), b.error
        assert [lv[0] for lv in b.levels] == g["levels"]
    with raftmc.ModelChecker(SYM_MC, plain, max_depth=6, workers=workers, **SMALL) as mc:
        mc.set_checkpoint(ck_plain, 1)
        assert mc.run().verdict == "DEPTH_LIMIT"
    for cfg, path in ((plain, ck), (cfgs["parity_trio"], ck_plain)):
        with raftmc.ModelChecker(SYM_MC, cfg, workers=workers, **SMALL) as mc:
            mc.set_recover(path)
            with pytest.raises(raftmc.RaftMCError) as e:
                mc.run()
        assert e.value.code == -1, str(e.value)


def test_first_five_server_election_under_symmetry(raftmc, tmp_path):
    """configs/c5e_noleader.cfg with SYMMETRY: TLC's single-worker first election at depth 14, as without
    symmetry, behind 3.7M orbits instead of 301.6M states (0.16 s measured, profiles/orig_symmetry.json).
    The counters are the host mirror's (tests/native/orig_sym_host.cpp, 2.6 CPU-minutes, not re-run
    here); the oracle's check-trace replays the trace against the cfg without the SYMMETRY line."""
    plain = os.path.join(CONFIGS, "c5e_noleader.cfg")
    cfg = sym_cfg("c5e_noleader")
    try:
        r = raftmc.check(SYM_MC, cfg, workers=1, fp_table_bytes=1 << 28, state_store_bytes=1 << 30)
    finally:
        os.unlink(cfg)
    assert (r.verdict, r.violated, r.depth, r.exit_code) == ("INVARIANT_VIOLATION", "NoLeader", 14, 12), r.error
    assert (r.generated, r.distinct) == (53631436, 3678428)
    assert [lv[0] for lv in r.levels] == [1, 2, 4, 13, 47, 164, 617, 2333, 9035, 34814, 129072, 429064, 1196577]
    assert r.actions["BecomeLeader"] == [1, 1] and r.actions["RequestVote"] == [19007433, 110627]
    states = trace_states(r)
    assert len(states) == 14 and "evoterLog |-> (" in states[-1]
    p = tmp_path / "trace.txt"
    p.write_text("\n".join(states) + "\n")
    o = run_oracle("check-trace", ORIG_MC, plain, "--golden", str(p))
    assert o["valid"] and o["violated"] == "NoLeader" and o["length"] == 14, o


def test_simulate_ignores_symmetry(raftmc, cfgs):
    """Walks use no fingerprints: the same seed gives the same walks with and without the line."""
    out = []
    for spec, cfg in ((ORIG_MC, os.path.join(CONFIGS, "parity_pair.cfg")), (SYM_MC, cfgs["parity_pair"])):
        with raftmc.ModelChecker(spec, cfg, seed=1, max_depth=32, **SMALL) as mc:
            r = mc.simulate(1024)
            out.append((r.verdict, r.generated, r.depth, r.actions, r.walks, r.steps, r.event_walk, mc.sim_walk(7)))
    assert out[0] == out[1] and out[0][4] == 1024
