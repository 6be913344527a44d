"""The starter seen-set of the single-GPU search (csrc/orig_backend.hip, ensure_starter): the search
begins on a small table while the full table's clear runs on a second stream, and orig_migrate
moves the entries to the full table at a level boundary.  RAFTMC_STARTER_SLOTS forces a tiny starter
so the switch happens on the small fixtures; every result must be what it is without the starter
(tests/golden/orig_parity.json, orig_events.json: bit-exact integer counts and the set of states).
"""
import json
import os
import re

import pytest

from oracle_util import CONFIGS, GOLDEN, ORIG_MC
from test_gpu import SMALL, _slot_bytes, states_sha, trace_states

pytestmark = pytest.mark.gpu

FIXTURES = json.load(open(os.path.join(GOLDEN, "orig_parity.json")))
EVENTS = json.load(open(os.path.join(GOLDEN, "orig_events.json")))
SWITCH = re.compile(r"seen-set switch after level (\d+): (\d+) entries moved")


def summary(r):
    return (r.verdict, r.generated, r.distinct, r.depth, r.left_on_queue, [lv[0] for lv in r.levels],
            {k: v[0] for k, v in r.actions.items()})


@pytest.mark.parametrize("workers", [1, 0])
@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_parity_across_a_switch(raftmc, monkeypatch, name, workers):
    """1024 starter slots: the half-load bound moves the seen-set to the full table within the first
    few levels, with probe clusters that wrap the starter's end; counts and states stay the oracle's."""
    monkeypatch.setenv("RAFTMC_STARTER_SLOTS", "1024")
    g = FIXTURES[name]
    with raftmc.ModelChecker(ORIG_MC, os.path.join(CONFIGS, name + ".cfg"), workers=workers, **SMALL) as mc:
        r = mc.run()
        sha, n = states_sha(mc)
    assert r.verdict == "OK", r.error
    assert (r.generated, r.distinct, r.depth) == (g["generated"], g["distinct"], g["depth"])
    assert [lv[0] for lv in r.levels] == g["levels"]
    if workers == 1:   # TLC's FIFO order: the kept producer of every state, so the distinct counts too
        assert r.actions == g["actions"]
    else:              # as test_parity_workers_n states
        assert {k: v[0] for k, v in r.actions.items()} == {k: v[0] for k, v in g["actions"].items()}
        assert sum(v[1] for v in r.actions.values()) == g["distinct"] - 1
    assert n == g["distinct"] and sha == g["states_sha256"]


@pytest.mark.parametrize("workers", [1, 0])
def test_the_switch_happened_and_moved_every_entry(raftmc, monkeypatch, capfd, workers):
    monkeypatch.setenv("RAFTMC_STARTER_SLOTS", "1024")
    monkeypatch.setenv("RAFTMC_PROGRESS", "1")
    g = FIXTURES["parity_pair"]
    capfd.readouterr()
    r = raftmc.check(ORIG_MC, os.path.join(CONFIGS, "parity_pair.cfg"), workers=workers, **SMALL)
    lines = SWITCH.findall(capfd.readouterr().err)
    assert r.verdict == "OK" and r.distinct == g["distinct"]
    assert len(lines) == 1, lines
    level, moved = int(lines[0][0]), int(lines[0][1])
    assert 0 < level < g["depth"]
    assert moved == sum(g["levels"][:level])


@pytest.mark.parametrize("workers", [1, 0])
def test_starter_disabled(raftmc, monkeypatch, capfd, workers):
    monkeypatch.setenv("RAFTMC_PROGRESS", "1")
    cfg = os.path.join(CONFIGS, "parity_pair.cfg")
    monkeypatch.setenv("RAFTMC_STARTER_SLOTS", "1024")
    a = raftmc.check(ORIG_MC, cfg, workers=workers, **SMALL)
    capfd.readouterr()
    monkeypatch.setenv("RAFTMC_STARTER_SLOTS", "0")
    with raftmc.ModelChecker(ORIG_MC, cfg, workers=workers, **SMALL) as mc:
        b = mc.run()
        sha, n = states_sha(mc)
    assert not SWITCH.findall(capfd.readouterr().err)
    assert summary(a) == summary(b)
    if workers == 1:
        assert a.actions == b.actions
    g = FIXTURES["parity_pair"]
    assert n == g["distinct"] and sha == g["states_sha256"]


def test_keys_survive_migration(raftmc, monkeypatch):
    """FIFO order: the ~key word travels with the fingerprint, so TLC's first-found producers, the
    stop point and the counterexample are unchanged."""
    monkeypatch.setenv("RAFTMC_STARTER_SLOTS", "1024")
    g = EVENTS["c2_noleader"]
    r = raftmc.check(ORIG_MC, os.path.join(CONFIGS, "c2_noleader.cfg"), workers=1, **SMALL)
    assert (r.verdict, r.violated) == (g["verdict"], g["violated"]), r.error
    assert (r.generated, r.distinct, r.left_on_queue, r.depth) == (g["generated"], g["distinct"], g["left_on_queue"], g["depth"])
    assert r.actions == g["actions"]
    assert trace_states(r) == [(t["action"], t["state"]) for t in g["trace"]]


@pytest.mark.parametrize("workers", [1, 0])
def test_run_that_ends_on_the_starter(raftmc, monkeypatch, capfd, workers):
    """c1 (3304 states) never outgrows 2^20 slots: the observed-collision scan reads the starter.  The
    minimum fingerprint gap depends only on the set, so it equals the value without the starter."""
    monkeypatch.setenv("RAFTMC_PROGRESS", "1")
    cfg = os.path.join(CONFIGS, "c1.cfg")
    vals = []
    for slots in (str(1 << 20), "0"):
        monkeypatch.setenv("RAFTMC_STARTER_SLOTS", slots)
        capfd.readouterr()
        with raftmc.ModelChecker(ORIG_MC, cfg, workers=workers, fp_table_bytes=1 << 30, state_store_bytes=1 << 28) as mc:
            r = mc.run()
            vals.append(mc.collision_observed())
        assert not SWITCH.findall(capfd.readouterr().err)
        assert r.verdict == "OK" and r.distinct == FIXTURES["c1"]["distinct"]
    assert 0 < vals[0] < 1
    assert vals[0] == vals[1]


@pytest.mark.parametrize("workers", [1, 0])
def test_overflow_is_still_reported(raftmc, monkeypatch, workers):
    monkeypatch.setenv("RAFTMC_STARTER_SLOTS", "256")
    r = raftmc.check(ORIG_MC, os.path.join(CONFIGS, "parity_pair.cfg"), workers=workers, fp_table_bytes=1 << 14,
                     state_store_bytes=1 << 26)
    assert r.verdict == "CAPACITY_OVERFLOW" and "fingerprint table full" in r.error, (r.verdict, r.error)


@pytest.mark.parametrize("workers", [1, 0])
def test_one_handle_twice(raftmc, monkeypatch, workers):
    monkeypatch.setenv("RAFTMC_STARTER_SLOTS", "1024")
    g = FIXTURES["parity_pair"]
    with raftmc.ModelChecker(ORIG_MC, os.path.join(CONFIGS, "parity_pair.cfg"), workers=workers, **SMALL) as mc:
        a = mc.run()
        b = mc.run()
        sha, n = states_sha(mc)
    assert summary(a) == summary(b)
    assert (a.verdict, a.generated, a.distinct) == ("OK", g["generated"], g["distinct"])
    assert n == g["distinct"] and sha == g["states_sha256"]


def test_small_store_with_starter(raftmc, monkeypatch):
    """test_stop_point_independent_of_chunking_and_spill's configuration (several chunks per level,
    completed levels spilled), starter forced: the same stop point."""
    monkeypatch.setenv("RAFTMC_STARTER_SLOTS", "1024")
    g = EVENTS["c2_noleader"]
    cfg = os.path.join(CONFIGS, "c2_noleader.cfg")
    cap = max(4 * 4096, 3 * max(g["levels"]))
    r = raftmc.check(ORIG_MC, cfg, fp_table_bytes=1 << 26, state_store_bytes=cap * _slot_bytes(raftmc, cfg))
    assert (r.verdict, r.generated, r.distinct, r.left_on_queue) == (g["verdict"], g["generated"], g["distinct"],
                                                                     g["left_on_queue"]), r.error
    assert r.actions == g["actions"]
    assert trace_states(r) == [(t["action"], t["state"]) for t in g["trace"]]


def test_recover_with_starter(raftmc, monkeypatch, tmp_path):
    """test_checkpoint_recover_c1's shape, starter forced: the checkpointed search switches tables, the
    recovered one starts on the full table, and it ends like the uninterrupted search."""
    monkeypatch.setenv("RAFTMC_STARTER_SLOTS", "1024")
    g = FIXTURES["c1"]
    cfg = os.path.join(CONFIGS, "c1.cfg")
    ck = str(tmp_path / "c1.ckpt")
    with raftmc.ModelChecker(ORIG_MC, cfg, max_depth=6, **SMALL) as mc:
        mc.set_checkpoint(ck, 1)
        a = mc.run()
    assert a.verdict == "DEPTH_LIMIT" and os.path.exists(ck)
    with raftmc.ModelChecker(ORIG_MC, cfg, **SMALL) as mc:
        mc.set_recover(ck)
        b = mc.run()
        sha, n = states_sha(mc)
    assert (b.verdict, b.generated, b.distinct, b.depth) == ("OK", g["generated"], g["distinct"], g["depth"])
    assert {k: v[0] for k, v in b.actions.items()} == {k: v[0] for k, v in g["actions"].items()}
    assert [lv[0] for lv in b.levels] == g["levels"]
    assert n == g["distinct"] and sha == g["states_sha256"]
