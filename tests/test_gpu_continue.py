"""Continue mode on the GPU (mc_set_continue, memb_witness.hip): one BFS reports the
first counterexample of every listed invariant.

The reference of every check is a fixture the project already has.  Invariants never decide which
states are explored and a violating state is still enqueued, so each witness of a continue run must
equal what the plain run listing that property alone reports -- depth, TLC's counters at the stop
point and the trace state by state -- and those single-property runs are oracle-pinned in
tests/golden/memb_parity.json ("scen_*", and "tlc:scen_*" in TLC's SYMMETRY rule).  Integer work:
the bar is equality."""
import json
import os
import subprocess

import pytest

from oracle_util import CONFIGS, GOLDEN, MEMB_MC, ORIG_MC, ROOT
from test_gpu_membership import EXIT, FIX, SMALL, _spill_store, open_case

pytestmark = pytest.mark.gpu

GROUPS = {
    "scen_all_shipped": ["BoundedTrace", "ConcurrentLeaders", "EntryCommitted", "FirstBecomeLeader", "FirstCommit", "FirstRestart",
                         "LeadershipChange"],
    "scen_all_dynamic3": ["AddCommits", "AddSucessful", "MembershipChange", "MembershipChangeCommits", "MultipleMembershipChanges"],
    "scen_all_grow2": ["MultipleMembershipChangesCommit", "LeaderChangesDuringConfChange"],
}
MODES = ["orbit", "tlc"]


def fixture_of(prop, mode):
    return FIX[("tlc:" if mode == "tlc" else "") + "scen_" + prop]


def continue_run(raftmc, cfg, mode, **kw):
    kw = dict(SMALL, deadlock=False, **kw)
    with raftmc.ModelChecker(MEMB_MC, os.path.join(CONFIGS, cfg + ".cfg"), sym_tlc=mode == "tlc", **kw) as mc:
        mc.set_continue()
        return mc.run()


def assert_witness_is_fixture(w, g):
    """test_scenario_shortest_counterexample's check, on one witness"""
    assert w.invariant == g["violated"]
    assert (w.depth, w.generated, w.distinct, w.left_on_queue) == (g["depth"], g["generated"], g["distinct"], g["left_on_queue"]), w
    blocks = w.trace_text.strip().split("\n\n")
    assert len(blocks) == len(g["trace"]) == g["depth"]
    for k, (blk, ref) in enumerate(zip(blocks, g["trace"])):
        head, *body = blk.split("\n")
        assert " ".join(body) == ref["state"], "%s: trace state %d differs" % (w.invariant, k + 1)
        if k:
            assert head == "State %d: <%s>" % (k + 1, ref["action"])


_RUNS = {}


def all_scenarios(raftmc, cfg, mode):
    """the one continue run of a group, shared by the tests that read it (never modified)"""
    if (cfg, mode) not in _RUNS:
        _RUNS[cfg, mode] = continue_run(raftmc, cfg, mode)
    return _RUNS[cfg, mode]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cfg", sorted(GROUPS))
def test_all_scenarios_in_one_run(raftmc, cfg, mode):
    r = all_scenarios(raftmc, cfg, mode)
    assert r.verdict == "INVARIANT_VIOLATION" and r.exit_code == 12, (r, r.error)
    assert sorted(w.invariant for w in r.witnesses) == sorted(GROUPS[cfg])     # one witness per listed property
    for w in r.witnesses:
        assert GROUPS[cfg][w.position] == w.invariant
        assert_witness_is_fixture(w, fixture_of(w.invariant, mode))
        assert w.actions == fixture_of(w.invariant, mode)["actions"]           # TLC's per-action counters at the same stop point
    # discovery order
    depths = [w.depth for w in r.witnesses]
    assert depths == sorted(depths)
    # the run's own summary is the last witness's, its counterexample the first witness's
    first, last = r.witnesses[0], r.witnesses[-1]
    assert (r.depth, r.generated, r.distinct, r.left_on_queue, r.actions) == (last.depth, last.generated, last.distinct, last.left_on_queue, last.actions)
    assert r.violated == first.invariant and r.trace_text == first.trace_text
    assert "memb_witness" in r.kernels and r.kernels["memb_witness"]["launches"] > 0


@pytest.mark.parametrize("mode", MODES)
def test_one_successor_is_the_witness_of_two_properties(raftmc, mode):
    """FirstCommit and EntryCommitted first fail on the same successor: cfg position breaks the tie"""
    r = all_scenarios(raftmc, "scen_all_shipped", mode)
    w = {x.invariant: x for x in r.witnesses}
    assert w["EntryCommitted"].trace_text == w["FirstCommit"].trace_text
    names = [x.invariant for x in r.witnesses]
    assert names.index("EntryCommitted") + 1 == names.index("FirstCommit")


@pytest.mark.parametrize("cfg,mode,case", [("scen_all_shipped", "orbit", "membership_shipped@14"),
                                           ("scen_all_shipped", "tlc", "tlc:membership_shipped@16"),
                                           ("scen_all_dynamic3", "orbit", "memb_dynamic3@14"),
                                           ("scen_all_dynamic3", "tlc", "tlc:memb_dynamic3@14")])
def test_continues_to_the_depth_limit(raftmc, cfg, mode, case):
    """Past every witness within reach, to max_depth: the plain search's counters (the fixture of the
    same model with invariants that hold), and exactly the witnesses no deeper than that."""
    g = FIX[case]
    r = continue_run(raftmc, cfg, mode, max_depth=g["max_depth"])
    assert (r.generated, r.distinct, r.depth, r.left_on_queue) == (g["generated"], g["distinct"], g["depth"], g["left_on_queue"]), r.error
    assert [lv[0] for lv in r.levels] == g["levels"]
    assert r.actions == g["actions"]
    want = sorted(p for p in GROUPS[cfg] if fixture_of(p, mode)["depth"] <= g["max_depth"])
    assert want and sorted(w.invariant for w in r.witnesses) == want
    for w in r.witnesses:
        assert_witness_is_fixture(w, fixture_of(w.invariant, mode))
    assert r.verdict == "INVARIANT_VIOLATION" and r.exit_code == 12
    assert r.violated == r.witnesses[0].invariant and r.trace_text == r.witnesses[0].trace_text


def test_nothing_violated_nothing_changed(raftmc):
    g = FIX["membership_shipped@14"]
    with open_case(raftmc, g, max_depth=g["max_depth"], **SMALL) as mc:
        mc.set_continue()
        r = mc.run()
    assert r.witnesses == [] and r.verdict == "DEPTH_LIMIT" and r.exit_code == 0, r.error
    assert (r.generated, r.distinct, r.depth, r.left_on_queue) == (g["generated"], g["distinct"], g["depth"], g["left_on_queue"])
    assert [lv[0] for lv in r.levels] == g["levels"]
    assert r.actions == g["actions"]


@pytest.mark.parametrize("case", ["eval:memb_eval_single", "deadlock:memb_unreliable"])
def test_fatal_events_end_the_run_as_they_end_a_plain_run(raftmc, case):
    """An invariant that fails to evaluate (the witness kernels' fatal slot) and a deadlock (the BFS
    kernels' own event): test_error_verdicts' checks with continue on."""
    g = FIX[case]
    with open_case(raftmc, g, **SMALL) as mc:
        mc.set_continue()
        r = mc.run()
    assert r.verdict == g["verdict"] and r.exit_code == EXIT[g["verdict"]], (r, r.error)
    assert (r.depth, r.generated, r.distinct, r.left_on_queue) == (g["depth"], g["generated"], g["distinct"], g["left_on_queue"])
    assert r.actions == g["actions"]
    blocks = r.trace_text.strip().split("\n\n")
    assert [" ".join(b.split("\n")[1:]) for b in blocks] == [t["state"] for t in g["trace"]]
    assert r.witnesses == []
    if g["verdict"] == "EVAL_ERROR":
        assert "Committed" in r.error and "Error:" in r.report
    else:
        assert "Deadlock reached" in r.report


def test_later_chunks_and_spilled_parents(raftmc):
    """A store sized by test_gpu_membership's _spill_store from the levels of tlc:scen_ConcurrentLeaders,
    the deepest search of the group: smaller than the search, so completed levels move to the host
    and (the chunk follows the store size) levels span several chunks; witnesses then come from later
    chunks and their traces cross the host/device split.
    The helper's margin: the store has to hold the last complete level (311,218 states) and the new
    states materialized before the stop (1,302,678 - 447,223 = 855,455), 2.86 times the largest pair
    of consecutive levels (408,194) that the helper scales, plus the rest of the stop's own chunk
    (about 25,000 parents with 3.2 new states each at that level, 0.2 of that pair); the fixture's
    1,302,678 distinct states are 3.19 times it.  So 3.1."""
    g = FIX["tlc:scen_ConcurrentLeaders"]
    store = _spill_store(raftmc, g, margin=3.1)
    r = continue_run(raftmc, "scen_all_shipped", "tlc", state_store_bytes=store)
    assert r.verdict == "INVARIANT_VIOLATION", r.error
    assert r.kernels["memb_expand"]["launches"] > 2 * len(g["levels"])      # levels took several chunks
    assert sorted(w.invariant for w in r.witnesses) == sorted(GROUPS["scen_all_shipped"])
    for w in r.witnesses:
        assert_witness_is_fixture(w, fixture_of(w.invariant, "tlc"))
    ref = all_scenarios(raftmc, "scen_all_shipped", "tlc")
    assert [(w.invariant, w.actions) for w in r.witnesses] == [(w.invariant, w.actions) for w in ref.witnesses]


def test_without_out_of_model_checks(raftmc):
    """MC_COMPAT_INV_OUT_OF_MODEL cleared (no fixture exists): every witness equals the plain
    single-property run with the same flag, taken here.
    FirstRestart needs a server that restarted twice, which BoundedRestarts keeps out of the model,
    so without the out-of-model checks it has no witness and neither search would end before the
    store is full: both stop at depth 19, the deepest witness of the group, where the plain
    FirstRestart run must report no violation either."""
    depth = max(fixture_of(p, "tlc")["depth"] for p in GROUPS["scen_all_shipped"])
    r = continue_run(raftmc, "scen_all_shipped", "tlc", inv_out_of_model=False, max_depth=depth)
    print(r, [(w.invariant, w.depth) for w in r.witnesses])
    assert r.verdict == "INVARIANT_VIOLATION", r.error
    assert sorted(w.invariant for w in r.witnesses) == sorted(p for p in GROUPS["scen_all_shipped"] if p != "FirstRestart")
    for p in GROUPS["scen_all_shipped"]:
        q = raftmc.check(MEMB_MC, os.path.join(CONFIGS, "scen_%s.cfg" % p), deadlock=False, sym_tlc=True, inv_out_of_model=False,
                         max_depth=depth, **SMALL)
        w = [x for x in r.witnesses if x.invariant == p]
        if not w:
            assert (q.verdict, q.violated) == ("DEPTH_LIMIT", ""), p
            assert (q.generated, q.distinct, q.left_on_queue, q.actions) == (r.generated, r.distinct, r.left_on_queue, r.actions)
            continue
        w = w[0]
        assert (q.verdict, q.violated) == ("INVARIANT_VIOLATION", p)
        assert (w.depth, w.generated, w.distinct, w.left_on_queue, w.actions, w.trace_text) == (
            q.depth, q.generated, q.distinct, q.left_on_queue, q.actions, q.trace_text), p


def test_refusals(raftmc, tmp_path):
    cfg = os.path.join(CONFIGS, "scen_all_shipped.cfg")
    with raftmc.ModelChecker(MEMB_MC, cfg, n_gpus=2, same_device=True, **SMALL) as mc:
        with pytest.raises(raftmc.RaftMCError) as e:
            mc.set_continue()
        assert e.value.code == -4
    import ctypes
    with raftmc.ModelChecker(MEMB_MC, cfg, **SMALL) as a, raftmc.ModelChecker(MEMB_MC, cfg, **SMALL) as b:
        a.set_continue()
        arr = (ctypes.c_void_p * 2)(a.h, b.h)
        assert a.lib.mc_shard_run_loopback(arr, 2) == -4
        assert a.lib.mc_shard_open(a.h, 0, 1) == -4
    with raftmc.ModelChecker(MEMB_MC, cfg, **SMALL) as mc:
        mc.set_continue()
        with pytest.raises(raftmc.RaftMCError) as e:
            mc.set_recover(str(tmp_path / "none.ckpt"))
        assert e.value.code == -4
    with raftmc.ModelChecker(ORIG_MC, os.path.join(CONFIGS, "c1.cfg"), **SMALL) as mc:
        mc.lib.mc_set_simulate(mc.h, 64, 0)
        with pytest.raises(raftmc.RaftMCError) as e:
            mc.set_continue()
        assert e.value.code == -4
    with raftmc.ModelChecker(MEMB_MC, cfg, **SMALL) as mc:
        mc.set_continue()
        assert mc.lib.mc_set_simulate(mc.h, 64, 0) == -4


def test_a_handle_that_never_asked_runs_the_plain_search(raftmc):
    g = FIX["scen_FirstCommit"]
    with open_case(raftmc, g, **SMALL) as mc:
        r = mc.run()
    assert (r.verdict, r.violated, r.exit_code) == ("INVARIANT_VIOLATION", "FirstCommit", 12)
    assert (r.depth, r.generated, r.distinct, r.left_on_queue) == (g["depth"], g["generated"], g["distinct"], g["left_on_queue"])
    assert r.witnesses == [] and "memb_witness" not in r.kernels


def test_cli_and_tlc_main(raftmc, capsys):
    exe = os.path.join(ROOT, "raft-tla_amd", "_build", "raftmc")
    args = ["-continue", "-deadlock", "-json", "-fptable", str(SMALL["fp_table_bytes"]), "-store", str(SMALL["state_store_bytes"]),
            "-config", os.path.join(CONFIGS, "scen_all_shipped.cfg"), MEMB_MC]
    p = subprocess.run([exe, *args], capture_output=True, text=True)
    assert p.returncode == 12, p.stderr
    ref = all_scenarios(raftmc, "scen_all_shipped", "tlc")       # the CLI's default is TLC's rule
    lines = p.stdout.strip().split("\n")
    errors = [l for l in lines if l.startswith("Error: Invariant ")]
    assert errors == ["Error: Invariant %s is violated." % w.invariant for w in ref.witnesses] and len(errors) == 7
    doc = json.loads(lines[-1])
    assert doc["witnesses"] == [{"invariant": w.invariant, "depth": w.depth, "generated": w.generated, "distinct": w.distinct}
                                for w in ref.witnesses]
    assert (doc["generated"], doc["distinct"], doc["depth"]) == (ref.generated, ref.distinct, ref.depth)
    # the Python entry point with TLC's argv
    code = raftmc.tlc_main(["-continue", "-deadlock", "-config", os.path.join(CONFIGS, "scen_all_grow2.cfg"), MEMB_MC])
    out = capsys.readouterr().out
    assert code == 12
    assert [l for l in out.split("\n") if l.startswith("Error: Invariant ")] == [
        "Error: Invariant MultipleMembershipChangesCommit is violated.", "Error: Invariant LeaderChangesDuringConfChange is violated."]
