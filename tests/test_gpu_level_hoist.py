"""The level hoist (csrc/orig_backend.hip launch_hoist, csrc/chunk_plan.h): a split
level of the single-GPU -workers N search generates the next level's first parents beside its own last
dedup, into the free half of the record buffers and a counter block of its own.  RAFTMC_OVERLAP_STATES
forces tiny sub-chunks and RAFTMC_HOIST_MIN=256 lets one workgroup's worth of parents be hoisted, so the
small fixtures hoist out of their levels from ~500 parents up, with prefixes from one workgroup to many
sub-chunks long; every result must be what it is without the hoist and on one stream
(tests/golden/orig_parity.json, orig_events.json: bit-exact integer counts and the set of states).
"""
import json
import os
import re

import pytest

from oracle_util import CONFIGS, GOLDEN, ORIG_MC
from test_gpu import SMALL, states_sha, trace_states

pytestmark = pytest.mark.gpu

FIXTURES = json.load(open(os.path.join(GOLDEN, "orig_parity.json")))
EVENTS = json.load(open(os.path.join(GOLDEN, "orig_events.json")))


@pytest.fixture
def hoist_env(monkeypatch):
    def set_env(sub, hoist="1", **more):
        monkeypatch.setenv("RAFTMC_OVERLAP_STATES", sub)
        monkeypatch.setenv("RAFTMC_HOIST_MIN", "256")
        monkeypatch.setenv("RAFTMC_HOIST", hoist)
        monkeypatch.setenv("RAFTMC_PROGRESS", "1")   # the handle reports its hoists on stderr
        for k, v in more.items():
            monkeypatch.setenv(k, v)
    return set_env


def hoists(capfd):
    """the hoists the runs since the last call launched: how many parents each"""
    return [int(n) for n in re.findall(r"^level hoist: (\d+) parents", capfd.readouterr().err, re.M)]


def summary(r):
    return (r.verdict, r.generated, r.distinct, r.depth, r.left_on_queue, [lv[0] for lv in r.levels],
            {k: v[0] for k, v in r.actions.items()}, sum(v[1] for v in r.actions.values()))


def check_golden(r, sha, n, g):
    assert r.verdict == "OK", r.error
    assert (r.generated, r.distinct, r.depth) == (g["generated"], g["distinct"], g["depth"])
    assert [lv[0] for lv in r.levels] == g["levels"]
    assert {k: v[0] for k, v in r.actions.items()} == {k: v[0] for k, v in g["actions"].items()}
    assert sum(v[1] for v in r.actions.values()) == g["distinct"] - 1
    assert n == g["distinct"] and sha == g["states_sha256"]


@pytest.mark.parametrize("starter", [None, "1024"])
@pytest.mark.parametrize("sub", ["256", "768"])
@pytest.mark.parametrize("name", ["parity_pair6", "parity_trio"])
def test_parity_hoisted(raftmc, hoist_env, capfd, name, sub, starter):
    """starter 1024: orig_migrate lands at a hoisted boundary, between the hoisted generate and the
    dedup of its records."""
    hoist_env(sub, **({"RAFTMC_STARTER_SLOTS": starter} if starter else {}))
    with raftmc.ModelChecker(ORIG_MC, os.path.join(CONFIGS, name + ".cfg"), workers=0, **SMALL) as mc:
        r = mc.run()
        sha, n = states_sha(mc)
    check_golden(r, sha, n, FIXTURES[name])
    each = hoists(capfd)
    # hoists happened: whole workgroups, RAFTMC_HOIST_MIN at the least, never more than the level holds
    assert each and all(x % 256 == 0 and 256 <= x <= max(FIXTURES[name]["levels"]) for x in each), each
    # the hoisted generate is counted where its chunk is: once per chunk, as ever
    assert r.kernels["orig_generate"]["launches"] == r.kernels["orig_materialize"]["launches"]


def test_hoist_off_equals_on(raftmc, hoist_env, capfd):
    cfg = os.path.join(CONFIGS, "parity_pair6.cfg")
    out = []
    for hoist in ("0", "1"):
        hoist_env("256", hoist)
        with raftmc.ModelChecker(ORIG_MC, cfg, workers=0, **SMALL) as mc:
            r = mc.run()
            out.append((summary(r), states_sha(mc)))
        assert bool(hoists(capfd)) == (hoist == "1")
    assert out[0] == out[1]
    check_golden(r, out[1][1][0], out[1][1][1], FIXTURES["parity_pair6"])


def test_event_behind_and_ahead_of_a_hoist(raftmc, hoist_env, capfd):
    """-workers N finds the event on a level whose first parents were generated ahead (its counters come
    through the fold), with the next hoist already queued: that one is given up, and the FIFO re-search
    gives TLC's verdict, counters and counterexample."""
    hoist_env("256")
    g = EVENTS["scenario_first_leader"]
    r = raftmc.check(ORIG_MC, os.path.join(CONFIGS, "scenario_first_leader.cfg"), workers=0, **SMALL)
    assert (r.verdict, r.violated) == (g["verdict"], g["violated"]), r.error
    assert (r.generated, r.distinct, r.left_on_queue, r.depth) == (g["generated"], g["distinct"], g["left_on_queue"], g["depth"])
    assert r.actions == g["actions"]
    assert trace_states(r) == [(t["action"], t["state"]) for t in g["trace"]]
    assert hoists(capfd)


@pytest.mark.parametrize("count_final", [False, True])
@pytest.mark.parametrize("max_depth", [11, 12])
def test_depth_limit_at_a_hoisted_boundary(raftmc, hoist_env, capfd, max_depth, count_final):
    """parity_pair6's level 10 (1960 parents) hoists into level 11 (3455): max_depth 11 stops at that
    boundary (no hoist may be left behind), 12 one level past it (with count_final_level the hoisted
    records feed the counted level).  Equal to the one-stream run."""
    cfg = os.path.join(CONFIGS, "parity_pair6.cfg")
    out = []
    for sub in ("0", "256"):
        hoist_env(sub)
        out.append(summary(raftmc.check(ORIG_MC, cfg, workers=0, max_depth=max_depth, count_final_level=count_final, **SMALL)))
        n = len(hoists(capfd))
        assert n == 0 if sub == "0" else n > 0
    assert out[0] == out[1]
    assert out[1][0] == "DEPTH_LIMIT" and out[1][3] == max_depth


def test_one_handle_twice_and_after_an_event(raftmc, hoist_env, capfd):
    """the second counter block, the generate stream and both halves are re-armed between runs, also
    behind a run that an event ended with a hoist queued"""
    hoist_env("256")
    g = FIXTURES["parity_pair6"]
    with raftmc.ModelChecker(ORIG_MC, os.path.join(CONFIGS, "parity_pair6.cfg"), workers=0, **SMALL) as mc:
        a = mc.run()
        b = mc.run()
        sha, n = states_sha(mc)
    assert summary(a) == summary(b)
    check_golden(b, sha, n, g)
    assert hoists(capfd)
    ev = EVENTS["scenario_first_leader"]
    with raftmc.ModelChecker(ORIG_MC, os.path.join(CONFIGS, "scenario_first_leader.cfg"), workers=0, **SMALL) as mc:
        a = mc.run()
        b = mc.run()
    assert a.verdict == b.verdict == ev["verdict"]
    assert (a.generated, a.distinct, a.left_on_queue, a.depth) == (b.generated, b.distinct, b.left_on_queue, b.depth) == \
        (ev["generated"], ev["distinct"], ev["left_on_queue"], ev["depth"])
    assert hoists(capfd)
