"""Generate beside dedup (csrc/orig_backend.hip run(), csrc/chunk_plan.h): the large levels of the
single-GPU -workers N search are cut into sub-chunks that alternate between two halves of the record
buffers, orig_generate of the next sub-chunk on a second stream beside the seen-set probes of this one.
RAFTMC_OVERLAP_STATES forces a tiny sub-chunk so that the small fixtures are pipelined from ~300
parents up, with both halves reused many times, a partial last sub-chunk and leader-work parents in
every half; every result must be what it is on one stream (tests/golden/orig_parity.json,
orig_events.json: bit-exact integer counts and the set of states).
"""
import json
import os

import pytest

from oracle_util import CONFIGS, GOLDEN, ORIG_MC
from test_gpu import SMALL, states_sha, trace_states

pytestmark = pytest.mark.gpu

FIXTURES = json.load(open(os.path.join(GOLDEN, "orig_parity.json")))
EVENTS = json.load(open(os.path.join(GOLDEN, "orig_events.json")))


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
def test_parity_pipelined(raftmc, monkeypatch, name, sub, starter):
    """starter 1024: orig_migrate lands in front of a pipelined level."""
    monkeypatch.setenv("RAFTMC_OVERLAP_STATES", sub)
    if starter:
        monkeypatch.setenv("RAFTMC_STARTER_SLOTS", starter)
    with raftmc.ModelChecker(ORIG_MC, os.path.join(CONFIGS, name + ".cfg"), workers=0, **SMALL) as mc:
        r = mc.run()
        sha, n = states_sha(mc)
    check_golden(r, sha, n, FIXTURES[name])
    # the levels were cut: every kernel but mark/scan ran once per sub-chunk
    g = FIXTURES[name]
    step = int(sub)
    want = sum((lv + step - 1) // step for lv in g["levels"])
    assert r.kernels["orig_generate"]["launches"] == want, (r.kernels, want)


def test_one_stream_equals_pipelined(raftmc, monkeypatch):
    cfg = os.path.join(CONFIGS, "parity_pair6.cfg")
    out = []
    for sub in ("0", "256"):
        monkeypatch.setenv("RAFTMC_OVERLAP_STATES", sub)
        with raftmc.ModelChecker(ORIG_MC, cfg, workers=0, **SMALL) as mc:
            r = mc.run()
            out.append((summary(r), states_sha(mc)))
    assert out[0] == out[1]
    check_golden(r, out[1][1][0], out[1][1][1], FIXTURES["parity_pair6"])


def test_event_under_overlap(raftmc, monkeypatch):
    """-workers N finds the event on a pipelined level and re-searches in FIFO order: TLC's verdict,
    counters and counterexample."""
    monkeypatch.setenv("RAFTMC_OVERLAP_STATES", "256")
    g = EVENTS["scenario_first_leader"]
    r = raftmc.check(ORIG_MC, os.path.join(CONFIGS, "scenario_first_leader.cfg"), workers=0, **SMALL)
    assert (r.verdict, r.violated) == (g["verdict"], g["violated"]), r.error
    assert (r.generated, r.distinct, r.left_on_queue, r.depth) == (g["generated"], g["distinct"], g["left_on_queue"], g["depth"])
    assert r.actions == g["actions"]
    assert trace_states(r) == [(t["action"], t["state"]) for t in g["trace"]]


def test_one_handle_twice(raftmc, monkeypatch):
    """buffers and counters are re-armed between runs"""
    monkeypatch.setenv("RAFTMC_OVERLAP_STATES", "256")
    g = FIXTURES["parity_pair6"]
    with raftmc.ModelChecker(ORIG_MC, os.path.join(CONFIGS, "parity_pair6.cfg"), workers=0, **SMALL) as mc:
        a = mc.run()
        b = mc.run()
        sha, n = states_sha(mc)
    assert summary(a) == summary(b)
    check_golden(b, sha, n, g)
