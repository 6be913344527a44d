"""Action properties ([][A]_vars) on raft_original on the GPU (configs/raft_original_actions_mc.tla,
DESIGN.md §14): the WithActions instantiations of the generate and simulate kernels through every path that
generates transitions.  The reference is tests/golden/orig_actions.json (the FIFO mirror of
tests/native/orig_actions_host.cpp, which checks the properties with a literal evaluator;
tests/golden/make_orig_actions.py); counterexamples are replayed by the CPU oracle's check-trace against the
cfg without its PROPERTIES line."""
import importlib
import json
import os

import pytest
import torch  # noqa: F401  (raft-tla_amd.shard's, imported before the library initialises HIP, as tests/test_gpu_shard.py does)

from oracle_util import CONFIGS, GOLDEN, ORIG_MC, cfg_variant
from test_orig_actions_host import (ACTIONS_MC, ACTIONS_SYM_MC, CONTROL, FAILING, FIXTURE, PARITY, SAFETY_FIXTURE, WIDE_COUNTS, actions_host,
                                    commit_regression, per_server, state_fields)
from test_orig_safety_host import ELEVEN
from test_sim_host import check_trace

pytestmark = pytest.mark.gpu

SMALL = dict(fp_table_bytes=1 << 26, state_store_bytes=1 << 28)
TRIO6 = dict(fp_table_bytes=1 << 28, state_store_bytes=1 << 30)   # 6.6M states
REGRESS = os.path.join(CONFIGS, "pair7_commit_regress.cfg")
PAIR7 = os.path.join(CONFIGS, "pair7.cfg")
STEPDOWN = os.path.join(CONFIGS, "parity_pair_stepdown.cfg")
PAIR_SHAPE = (2, 1, 2, 1, 5)
WALKS = (0, 63, 64, 1023, 1024, 4095)   # a wave edge, a batch edge, the last walk
# cfg with the four holding properties -> (the same model without them, its wrapper, the fixture with its counts)
HOLDING_MODELS = {"parity_pair_actions": ("parity_pair", PARITY["parity_pair"], SMALL), "c1_actions": ("c1", PARITY["c1"], SMALL),
                  "pair6_actions": ("pair6_nocommit", SAFETY_FIXTURE["pair6_nocommit"], SMALL),
                  "safety_trio6_actions": ("safety_trio6", SAFETY_FIXTURE["safety_trio6"], TRIO6)}


def trace_states(r):
    return [" ".join(blk.split("\n")[1:]) for blk in r.trace_text.strip().split("\n\n")]


def at_fixture_stop_point(r, g):
    assert (r.verdict, r.violated, r.exit_code) == (g["verdict"], g["violated"], 12), r.error
    assert (r.depth, r.generated, r.distinct, r.left_on_queue) == (g["depth"], g["generated"], g["distinct"], g["left_on_queue"])
    assert r.actions == g["actions"]
    assert [lv[0] for lv in r.levels] == g["levels"]
    states = trace_states(r)
    assert states == g["trace"] and len(states) == g["depth"]
    assert "Error: Action property %s is violated.\nError: The behavior up to this point is:\nState 1: <Initial predicate>" % g["violated"] in r.report
    assert "Verdict: ACTION_PROPERTY_VIOLATION" in r.report


def pair7_oracle_cfg(wide):
    """pair7.cfg (no PROPERTIES) for check-trace; wide: message counts in -1..2, under which the out-of-model
    last state of the counterexample is in the model (test_orig_actions_host.test_counterexamples_are_behaviours)"""
    return cfg_variant(PAIR7, replace=WIDE_COUNTS if wide else [])


def test_commit_regression_in_tlc_order(raftmc):
    """pair7_commit_regress.cfg, -workers 1, MC_COMPAT_INV_OUT_OF_MODEL set: TLC's single-worker stop point -- a
    HandleAppendEntriesRequest step into an out-of-model successor -- with the fixture's counters, per-action
    counts and trace, state by state."""
    g = FIXTURE["pair7_commit_regress"]
    assert (g["verdict"], g["violated"]) == ("ACTION_PROPERTY_VIOLATION", FAILING)
    r = raftmc.check(ACTIONS_MC, REGRESS, workers=1, **SMALL)
    at_fixture_stop_point(r, g)
    assert commit_regression(*trace_states(r)[-2:])


def test_commit_regression_level_parallel(raftmc, tmp_path):
    g = FIXTURE["pair7_commit_regress"]
    r = raftmc.check(ACTIONS_MC, REGRESS, workers=0, **SMALL)
    assert (r.verdict, r.violated, r.exit_code, r.depth) == ("ACTION_PROPERTY_VIOLATION", FAILING, 12, g["depth"]), r.error
    states = trace_states(r)
    cfg = pair7_oracle_cfg(True)
    try:
        o = check_trace(cfg, states, tmp_path)
    finally:
        os.unlink(cfg)
    assert o["bad_step"] == -1 and o["violated"] == "" and o["length"] == len(states) == g["depth"], o
    assert commit_regression(*states[-2:])


def test_commit_regression_into_a_seen_state(raftmc):
    """The same with MC_COMPAT_INV_OUT_OF_MODEL cleared: the first violating in-model transition leads to a
    state already in the seen-set, which no materialize kernel ever sees -- the fixture's second stop point."""
    g = FIXTURE["pair7_commit_regress_inmodel"]
    assert g["inv_out_of_model"] is False and g["depth"] == 21
    r = raftmc.check(ACTIONS_MC, REGRESS, workers=1, inv_out_of_model=False, **SMALL)
    at_fixture_stop_point(r, g)


@pytest.mark.parametrize("workers", [1, 0])
@pytest.mark.parametrize("name", list(HOLDING_MODELS))
def test_holding_properties_change_nothing(raftmc, name, workers):
    """The four holding properties: verdict OK, and the counts, levels and per-action counts of the existing
    fixtures and of the same handle's model without them; then with the eleven §12 invariants listed too
    (WithActions<WithSafety<S>>)."""
    base, ref, sizes = HOLDING_MODELS[name]
    g = FIXTURE[name]
    assert g["verdict"] == "OK" and (g["generated"], g["distinct"], g["depth"], g["levels"]) == (ref["generated"], ref["distinct"], ref["depth"], ref["levels"])
    cfg = os.path.join(CONFIGS, name + ".cfg")
    plain_cfg = cfg_variant(os.path.join(CONFIGS, base + ".cfg"), replace=[("    NoCommit\n", "")] if base == "pair6_nocommit" else [])
    listed = open(cfg).read().split("INVARIANTS\n")[1].split("PROPERTIES\n")[0].split()
    both_cfg = cfg_variant(cfg, replace=[("INVARIANTS\n", "INVARIANTS\n" + "".join("    %s\n" % n for n in ELEVEN if n not in listed))])
    try:
        r = raftmc.check(ACTIONS_MC, cfg, workers=workers, **sizes)
        plain = raftmc.check(ORIG_MC, plain_cfg, workers=workers, **sizes)
        both = raftmc.check(ACTIONS_MC, both_cfg, workers=workers, **sizes)
    finally:
        os.unlink(plain_cfg)
        os.unlink(both_cfg)
    print(name, workers, "seconds", r.seconds, plain.seconds, both.seconds)
    for x in (r, plain, both):
        assert x.verdict == "OK", (x.violated, x.error)
        assert (x.generated, x.distinct, x.depth) == (g["generated"], g["distinct"], g["depth"])
        assert [lv[0] for lv in x.levels] == g["levels"]
        assert {k: v[0] for k, v in x.actions.items()} == {k: v[0] for k, v in g["actions"].items()}
        assert list(x.kernels) == list(plain.kernels)
    if workers == 1:
        assert r.actions == plain.actions == both.actions == g["actions"]


def test_control_in_tlc_order(raftmc, tmp_path):
    g = FIXTURE["parity_pair_stepdown"]
    r = raftmc.check(ACTIONS_MC, STEPDOWN, workers=1, **SMALL)
    assert g["violated"] == CONTROL
    at_fixture_stop_point(r, g)


@pytest.mark.parametrize("workers", [1, 0])
def test_with_symmetry(raftmc, workers, tmp_path):
    """SYMMETRY ServerSymmetry: on c1 the holding four give §11's orbit counts; the control is still found (on
    parity_pair: c1's two messages never elect a leader) and its trace is a behaviour of parity_pair.cfg whose
    last step takes a leader's leadership."""
    g = json.load(open(os.path.join(GOLDEN, "orig_symmetry.json")))["c1"]
    assert (g["generated"], g["distinct"], g["depth"]) == (9334, 611, 12)
    cfg = cfg_variant(os.path.join(CONFIGS, "c1_actions.cfg"), append="SYMMETRY ServerSymmetry\n")
    pair = os.path.join(CONFIGS, "parity_pair.cfg")
    ctl = cfg_variant(STEPDOWN, append="SYMMETRY ServerSymmetry\n")
    try:
        r = raftmc.check(ACTIONS_SYM_MC, cfg, workers=workers, **SMALL)
        c = raftmc.check(ACTIONS_SYM_MC, ctl, workers=workers, **SMALL)
    finally:
        os.unlink(cfg)
        os.unlink(ctl)
    assert r.verdict == "OK", (r.violated, r.error)
    assert (r.generated, r.distinct, r.depth) == (g["generated"], g["distinct"], g["depth"])
    assert [lv[0] for lv in r.levels] == g["levels"]
    assert (c.verdict, c.violated, c.exit_code) == ("ACTION_PROPERTY_VIOLATION", CONTROL, 12), c.error
    states = trace_states(c)
    o = check_trace(pair, states, tmp_path)
    # (a Restart step stays in the model; an UpdateTerm step too)
    assert o["bad_step"] == -1 and o["violated"] == "" and o["length"] == len(states) == c.depth, o
    a, b = per_server(state_fields(states[-2])["state"]), per_server(state_fields(states[-1])["state"])
    assert any(a[s] == "Leader" and b[s] != "Leader" for s in a), states[-2:]


def test_simulation_equals_the_host_mirror(raftmc):
    """Seed 1, 4096 walks of depth 32 in batches of 1024 on parity_pair with the control: generated, steps,
    walks, the event walk and the event's trace equal the mirror's (orig_sim_host.cpp's rules plus the
    literal property check) bit for bit, and the walks at a wave edge, a batch edge and the end are the
    mirror's line for line.  The mirror finds its event in the first batch: 4096 walks suffice."""
    host = actions_host(PAIR_SHAPE, "sim", STEPDOWN, 1, 4096, 32, 1024)
    assert host["event"] is not None and host["walks"] == 1024, host
    with raftmc.ModelChecker(ACTIONS_MC, STEPDOWN, seed=1, max_depth=32, **SMALL) as mc:
        r = mc.simulate(4096, 1024)
        walks = {w: mc.sim_walk(w) for w in WALKS}
    print("gpu", r.generated, r.steps, r.walks, r.event_walk, "host", host["generated"], host["steps"], host["walks"], host["event"])
    assert (r.verdict, r.violated, r.exit_code) == ("ACTION_PROPERTY_VIOLATION", CONTROL, 12), r.error
    assert (r.generated, r.steps, r.walks, r.depth) == (host["generated"], host["steps"], host["walks"], host["depth"])
    assert {k: v[0] for k, v in r.actions.items()} == host["actions"]
    assert r.event_walk == host["event"]["walk"]
    states = trace_states(r)
    assert len(states) == host["event"]["length"]
    mirror_walk = lambda w: actions_host_lines(PAIR_SHAPE, "sim", STEPDOWN, 1, 1, 32, 1, "--walk", w)   # noqa: E731
    assert states == mirror_walk(r.event_walk)
    for w in WALKS:
        assert walks[w] == mirror_walk(w), w


def actions_host_lines(shape, *args):
    import subprocess
    from test_orig_actions_host import make_orig_actions
    out = subprocess.run([make_orig_actions.build_actions_host(shape), *map(str, args)], capture_output=True, text=True, check=True, timeout=600).stdout
    return out.strip().split("\n")


def test_checkpoint_recover(raftmc, tmp_path):
    """A checkpoint at level 8 of pair7 with CommitIndexMonotonic recovers to the uninterrupted stop point; the
    properties are part of the checkpoint's model identity."""
    g = FIXTURE["pair7_commit_regress"]
    ck = str(tmp_path / "actions.ckpt")
    with raftmc.ModelChecker(ACTIONS_MC, REGRESS, max_depth=8, workers=1, **SMALL) as mc:
        mc.set_checkpoint(ck, 1)
        a = mc.run()
    assert a.verdict == "DEPTH_LIMIT" and a.depth == 8 and os.path.exists(ck)
    with raftmc.ModelChecker(ACTIONS_MC, REGRESS, workers=1, **SMALL) as mc:
        mc.set_recover(ck)
        b = mc.run()
    at_fixture_stop_point(b, g)
    with raftmc.ModelChecker(ACTIONS_MC, PAIR7, workers=1, **SMALL) as mc:
        mc.set_recover(ck)
        with pytest.raises(raftmc.RaftMCError) as e:
            mc.run()
    assert e.value.code == -1, str(e.value)   # MC_E_INVALID
    # ... nor the reverse: a checkpoint written without properties into a handle that lists one
    ck2 = str(tmp_path / "plain.ckpt")
    with raftmc.ModelChecker(ACTIONS_MC, PAIR7, max_depth=8, workers=1, **SMALL) as mc:
        mc.set_checkpoint(ck2, 1)
        assert mc.run().verdict == "DEPTH_LIMIT" and os.path.exists(ck2)
    with raftmc.ModelChecker(ACTIONS_MC, REGRESS, workers=1, **SMALL) as mc:
        mc.set_recover(ck2)
        with pytest.raises(raftmc.RaftMCError) as e:
            mc.run()
    assert e.value.code == -1, str(e.value)


def test_loopback_two_ranks(raftmc):
    """The sharded native loop runs the same generate kernels: two loopback ranks report the single-GPU
    -workers N verdict, name and depth."""
    shard = importlib.import_module("raft-tla_amd.shard")
    g = FIXTURE["pair7_commit_regress"]
    single = raftmc.check(ACTIONS_MC, REGRESS, workers=0, **SMALL)
    assert (single.verdict, single.violated, single.depth) == (g["verdict"], g["violated"], g["depth"])
    for r in shard.check_loopback(ACTIONS_MC, REGRESS, 2, workers=0, **SMALL):
        assert (r.verdict, r.violated, r.depth) == (single.verdict, single.violated, single.depth), r.error
