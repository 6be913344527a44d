"""Raft's log- and commit-safety invariants on raft_original on the GPU
(configs/raft_original_safety_mc.tla): the WithSafety instantiations of the generate,
materialize and simulate kernels through every path that checks invariants.  The reference is
tests/golden/orig_safety.json (the generated front end's host BFS over the unmodified reference
text, tests/golden/make_orig_safety.py); counterexamples are replayed by the CPU oracle's check-trace
against configs/safety_trio6.cfg, which lists none of the new names, plus NoCommit: check-trace calls a
trace valid when its last state, and no earlier one, violates an invariant of the cfg, and the oracle
knows NoCommit -- which the control's counterexamples, ending at a walk's first commit, violate there."""
import importlib
import json
import os

import pytest
import torch  # noqa: F401  (raft-tla_amd.shard's, imported before the library initialises HIP, as tests/test_gpu_shard.py does)

from oracle_util import CONFIGS, GOLDEN, ORIG_MC, cfg_variant
from test_orig_safety_host import CONTROL, ELEVEN, FIXTURE, SAFETY_MC, safety_cfg
from test_sim_host import check_trace

pytestmark = pytest.mark.gpu

SMALL = dict(fp_table_bytes=1 << 26, state_store_bytes=1 << 28)
TRIO6 = dict(fp_table_bytes=1 << 28, state_store_bytes=1 << 30)   # 6.6M states
SAFETY_SYM_MC = os.path.join(CONFIGS, "raft_original_safety_sym_mc.tla")
SMALL_MODELS = ["c1", "pair6_nocommit", "parity_pair"]
# -simulate on safety_trio6 with the control: seed 1, walks of at most 100 states.  The host replay of
# the same draws (tests/native/orig_sim_host.cpp's rule with the safety invariants) finds its first
# violation on walk 92874, after 51 states, in the first batch of 262144 walks (the default batch).
SIM_SEED, SIM_DEPTH, SIM_WALKS, SIM_EVENT_WALK, SIM_EVENT_STATES = 1, 100, 1 << 18, 92874, 51


@pytest.fixture(scope="module")
def cfgs():
    """entry -> its cfg with the fixture's INVARIANTS, plus "<name>:plain" with the two old ones (temp
    files, removed at the end of the module)"""
    paths = {e: safety_cfg(g["cfg"], g["invariants"]) for e, g in FIXTURE.items()}
    for name in SMALL_MODELS:
        paths[name + ":plain"] = safety_cfg(name, ELEVEN[:2])
    yield paths
    for p in paths.values():
        os.unlink(p)


@pytest.fixture(scope="module")
def oracle_cfg():
    """configs/safety_trio6.cfg (no control, none of the new names) plus NoCommit, for check-trace"""
    path = cfg_variant(os.path.join(CONFIGS, "safety_trio6.cfg"), append="    NoCommit\n")
    yield path
    os.unlink(path)


def trace_states(r):
    return [" ".join(blk.split("\n")[1:]) for blk in r.trace_text.strip().split("\n\n")]


@pytest.mark.parametrize("workers", [1, 0])
@pytest.mark.parametrize("name", SMALL_MODELS)
def test_counts_equal_the_fixture(raftmc, cfgs, name, workers):
    """All eleven invariants hold on the three small models: the fixture's counts and levels, and the
    per-action counts of the same search without the new names (which launches the kernels compiled
    without them)."""
    g = FIXTURE[name]
    assert g["invariants"] == ELEVEN and g["verdict"] == "OK"
    r = raftmc.check(SAFETY_MC, cfgs[name], workers=workers, **SMALL)
    assert r.verdict == "OK", (r.violated, r.error)
    assert (r.generated, r.distinct, r.depth) == (g["generated"], g["distinct"], g["depth"])
    assert [lv[0] for lv in r.levels] == g["levels"]
    plain = raftmc.check(ORIG_MC, cfgs[name + ":plain"], workers=workers, **SMALL)
    assert plain.verdict == "OK" and {k: v[0] for k, v in r.actions.items()} == {k: v[0] for k, v in plain.actions.items()}
    assert sum(v[0] for v in r.actions.values()) == g["generated"] - 1
    if workers == 1:
        assert r.actions == plain.actions
    assert list(r.kernels) == list(plain.kernels)


@pytest.mark.parametrize("workers", [1, 0])
def test_safety_trio6_full_search(raftmc, cfgs, workers):
    """The smallest 3-server model with commits, all eleven: no violation in 6.6M states."""
    g = FIXTURE["safety_trio6"]
    assert g["invariants"] == ELEVEN
    r = raftmc.check(SAFETY_MC, cfgs["safety_trio6"], workers=workers, **TRIO6)
    print("safety_trio6 workers=%d: %.3f s, %.3f s in kernels" % (workers, r.seconds, r.kernel_seconds))
    assert (r.verdict, r.violated) == (g["verdict"], g["violated"]), r.error
    assert (r.generated, r.distinct, r.depth) == (g["generated"], g["distinct"], g["depth"])
    assert [lv[0] for lv in r.levels] == g["levels"]


def test_control_counterexample_in_tlc_order(raftmc, cfgs, oracle_cfg, tmp_path):
    """AllHaveCommitted_false alone, workers=1: TLC's single-worker stop point (the first commit, which
    leaves s3 without the entry) with the fixture's counters and its trace state by state; the oracle
    accepts the trace as a behaviour of safety_trio6.cfg."""
    g = FIXTURE["safety_trio6_control"]
    r = raftmc.check(SAFETY_MC, cfgs["safety_trio6_control"], workers=1, **TRIO6)
    assert (r.verdict, r.violated, r.exit_code) == ("INVARIANT_VIOLATION", CONTROL, 12), r.error
    assert (g["verdict"], g["violated"]) == ("INVARIANT_VIOLATION", CONTROL)
    assert (r.depth, r.generated, r.distinct, r.left_on_queue) == (g["depth"], g["generated"], g["distinct"], g["left_on_queue"])
    assert [lv[0] for lv in r.levels] == g["levels"][:-1]   # (the fixture also counts the stopped level's new states)
    states = trace_states(r)
    assert states == g["trace"] and len(states) == g["depth"]
    o = check_trace(oracle_cfg, states, tmp_path)
    assert o["valid"] and o["violated"] == "NoCommit" and o["length"] == len(states), o


def test_control_counterexample_level_parallel(raftmc, cfgs, oracle_cfg, tmp_path):
    g = FIXTURE["safety_trio6_control"]
    r = raftmc.check(SAFETY_MC, cfgs["safety_trio6_control"], workers=0, **TRIO6)
    assert (r.verdict, r.violated, r.exit_code, r.depth) == ("INVARIANT_VIOLATION", CONTROL, 12, g["depth"]), r.error
    states = trace_states(r)
    o = check_trace(oracle_cfg, states, tmp_path)
    assert o["valid"] and o["violated"] == "NoCommit" and o["length"] == len(states) == g["depth"], o


@pytest.mark.parametrize("workers", [1, 0])
def test_with_symmetry(raftmc, workers):
    """SYMMETRY ServerSymmetry plus all eleven on c1 (every safety invariant is permutation-invariant):
    OK with the orbit counts of tests/golden/orig_symmetry.json."""
    g = json.load(open(os.path.join(GOLDEN, "orig_symmetry.json")))["c1"]
    cfg = safety_cfg("c1", ELEVEN, append="SYMMETRY ServerSymmetry\n")
    try:
        r = raftmc.check(SAFETY_SYM_MC, cfg, workers=workers, **SMALL)
    finally:
        os.unlink(cfg)
    assert r.verdict == "OK", (r.violated, r.error)
    assert (r.generated, r.distinct, r.depth) == (g["generated"], g["distinct"], g["depth"])
    assert [lv[0] for lv in r.levels] == g["levels"]


def test_simulate_finds_the_control(raftmc, cfgs, oracle_cfg, tmp_path):
    cfg = cfgs["safety_trio6_control"]
    with raftmc.ModelChecker(SAFETY_MC, cfg, seed=SIM_SEED, max_depth=SIM_DEPTH, **SMALL) as mc:
        r = mc.simulate(SIM_WALKS)
    print("simulate: %d walks, %d steps, event walk %d, trace of %d states" % (r.walks, r.steps, r.event_walk, r.depth))
    assert (r.verdict, r.violated, r.exit_code) == ("INVARIANT_VIOLATION", CONTROL, 12), (r, r.error)
    states = trace_states(r)
    assert (r.event_walk, len(states)) == (SIM_EVENT_WALK, SIM_EVENT_STATES)
    o = check_trace(oracle_cfg, states, tmp_path)
    assert o["valid"] and o["violated"] == "NoCommit" and o["length"] == len(states), o


@pytest.mark.parametrize("workers", [1, 0])
def test_checkpoint_recover(raftmc, cfgs, tmp_path, workers):
    """pair6_nocommit with all eleven stopped at level 8 with a checkpoint per level resumes to the
    uninterrupted result; the names are part of the checkpoint's model identity."""
    g = FIXTURE["pair6_nocommit"]
    ck = str(tmp_path / "safety.ckpt")
    with raftmc.ModelChecker(SAFETY_MC, cfgs["pair6_nocommit"], max_depth=8, workers=workers, **SMALL) as mc:
        mc.set_checkpoint(ck, 1)
        a = mc.run()
    assert a.verdict == "DEPTH_LIMIT" and a.depth == 8 and os.path.exists(ck)
    with raftmc.ModelChecker(SAFETY_MC, cfgs["pair6_nocommit"], workers=workers, **SMALL) as mc:
        mc.set_recover(ck)
        b = mc.run()
    assert (b.verdict, b.generated, b.distinct, b.depth) == ("OK", g["generated"], g["distinct"], g["depth"]), b.error
    assert [lv[0] for lv in b.levels] == g["levels"]
    with raftmc.ModelChecker(ORIG_MC, cfgs["pair6_nocommit:plain"], workers=workers, **SMALL) as mc:
        mc.set_recover(ck)
        with pytest.raises(raftmc.RaftMCError) as e:
            mc.run()
    assert e.value.code == -1, str(e.value)


def test_loopback_two_ranks(raftmc, cfgs):
    """The sharded native loop (orig_materialize_sh) on two loopback ranks: the single-GPU counts."""
    shard = importlib.import_module("raft-tla_amd.shard")
    g = FIXTURE["pair6_nocommit"]
    for r in shard.check_loopback(SAFETY_MC, cfgs["pair6_nocommit"], 2, workers=0, **SMALL):
        assert r.verdict == "OK", (r.violated, r.error)
        assert (r.generated, r.distinct, r.depth) == (g["generated"], g["distinct"], g["depth"])
        assert [lv[0] for lv in r.levels] == g["levels"]
