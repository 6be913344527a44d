"""Action properties ([][A]_vars) on raft_original (configs/raft_original_actions_mc.tla) on
the host (no GPU): the packed evaluation the kernels compile (csrc/orig_spec.h violated_action, act_frame)
against a literal evaluator of each definition (tests/native/orig_actions_host.cpp), the FIFO mirror that
wrote tests/golden/orig_actions.json (tests/golden/make_orig_actions.py) run again, its counterexamples
replayed by the CPU oracle's check-trace, and the boundary (mc_open)."""
import importlib.util
import json
import os

import pytest

from oracle_util import CONFIGS, GOLDEN, ORIG_MC, cfg_variant
from test_sim_host import check_trace

_spec = importlib.util.spec_from_file_location("make_orig_actions", os.path.join(GOLDEN, "make_orig_actions.py"))
make_orig_actions = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(make_orig_actions)
actions_host, RUNS = make_orig_actions.actions_host, make_orig_actions.RUNS

ACTIONS_MC = os.path.join(CONFIGS, "raft_original_actions_mc.tla")
ACTIONS_SYM_MC = os.path.join(CONFIGS, "raft_original_actions_sym_mc.tla")
FIXTURE = json.load(open(os.path.join(GOLDEN, "orig_actions.json")))
PARITY = json.load(open(os.path.join(GOLDEN, "orig_parity.json")))
SAFETY_FIXTURE = json.load(open(os.path.join(GOLDEN, "orig_safety.json")))
HOLDING = ["TermsMonotonic", "OneVotePerTerm", "LeaderAppendOnly", "CommittedNeverLost"]
FAILING = "CommitIndexMonotonic"
CONTROL = "LeaderNeverStepsDown_false"
SIX = HOLDING + [FAILING, CONTROL]
# cfg -> shape (N, NV, MaxTerm, MaxLogLen, MaxMsgDomain) of the models whose every reachable transition is compared
CHECKED = {"parity_pair": (2, 1, 2, 1, 5), "pair6_nocommit": (2, 1, 2, 1, 6), "c1": (3, 1, 2, 1, 2), "parity_trio": (3, 2, 3, 2, 2),
           "pair7": (2, 1, 2, 1, 7)}
# (distinct, generated) of each: tests/golden/orig_parity.json, orig_safety.json, orig_actions.json
COUNTS = {"parity_pair": (20938, 408109), "pair6_nocommit": (85322, 1906605), "c1": (3304, 50740), "parity_trio": (42546, 673141),
          "pair7": (310858, 7774637)}
MUTATIONS = 8
WIDE_COUNTS = [("MinMsgCount = 0", "MinMsgCount = -1"), ("MaxMsgCount = 1", "MaxMsgCount = 2")]
VIOLATED = ["pair7_commit_regress", "pair7_commit_regress_inmodel", "parity_pair_stepdown"]


def state_fields(line):
    """a canonical state line -> {variable: text}"""
    out = {}
    for part in line.split("/\\ ")[1:]:
        name, _, val = part.partition(" = ")
        out[name.strip()] = val.strip()
    return out


def per_server(text):
    """(s1 :> 0 @@ s2 :> 1) -> {"s1": "0", "s2": "1"}"""
    return dict(p.split(" :> ") for p in text.strip("()").split(" @@ "))


def commit_regression(prev, last):
    """the servers whose commitIndex drops in the step while the step is not their Restart: a restart
    leaves the server's commitIndex 0, its state Follower and the message bag as it was"""
    a, b = state_fields(prev), state_fields(last)
    ca, cb = per_server(a["commitIndex"]), per_server(b["commitIndex"])
    out = []
    for s in ca:
        restart = int(cb[s]) == 0 and per_server(b["state"])[s] == "Follower" and a["messages"] == b["messages"]
        if int(cb[s]) < int(ca[s]) and not restart:
            out.append(s)
    return out


@pytest.fixture(scope="module")
def host_checks():
    """cfg -> the harness's `check` report over the model's every reachable transition, computed once"""
    return {name: actions_host(shape, "check", os.path.join(CONFIGS, name + ".cfg"), "--mutations", MUTATIONS, "--seed", 1)
            for name, shape in CHECKED.items()}


@pytest.fixture(scope="module")
def mirror_runs():
    """fixture entry -> the FIFO mirror run again (all but safety_trio6_actions: 70 s, the make script's)"""
    out = {}
    for entry, (cfg, shape, extra) in RUNS.items():
        if entry != "safety_trio6_actions":
            out[entry] = actions_host(shape, "bfs", os.path.join(CONFIGS, cfg + ".cfg"), *extra)
    return out


def test_packed_evaluation_equals_the_literal_definitions(host_checks):
    """(a) Every reachable transition of the five models, out-of-model successors included, and MUTATIONS
    seeded mutated successors per transition: S::violated_action equals the literal evaluator bit for bit,
    and each of the six properties is violated on some compared pair and holds on some."""
    total = {n: [0, 0] for n in SIX}
    for name, c in host_checks.items():
        print(name, json.dumps(c))
        assert (c["states"], c["transitions"]) == (COUNTS[name][0], COUNTS[name][1] - 1), c
        assert c["compared"] == (1 + MUTATIONS) * c["transitions"] and c["disagreements"] == 0, c
        for n, (t, f) in c["properties"].items():
            total[n][0] += t
            total[n][1] += f
    assert sorted(total) == sorted(SIX)
    assert all(t > 0 and f > 0 for t, f in total.values()), total
    assert PARITY["parity_trio"]["distinct"] == COUNTS["parity_trio"][0] and FIXTURE["pair7"]["distinct"] == COUNTS["pair7"][0]


def test_frame_conditions_hold_on_every_reachable_transition(host_checks):
    """(b) On every reachable transition the mask over all six under act_frame(action) equals the full mask,
    and every step of a Restart(i) instance satisfies the formula Restart(i) (so leaving Restart out of
    CommitIndexMonotonic's frame loses nothing): 0 outside the frames."""
    for name, c in host_checks.items():
        assert c["frame_checked"] == COUNTS[name][1] - 1 and c["frame_bad"] == 0 and c["restart_steps"] > 0, (name, c)


def test_fifo_mirror_reproduces_the_fixture(mirror_runs):
    """(c) tests/golden/orig_actions.json is what the mirror computes, and where no property is violated the
    counts are those of the fixtures written by other implementations."""
    for entry, r in mirror_runs.items():
        g = FIXTURE[entry]
        for k in ("verdict", "violated", "generated", "distinct", "left_on_queue", "depth", "levels", "actions"):
            assert r[k] == g[k], (entry, k)
        if g["verdict"] != "OK":
            assert [s["state"] for s in r["trace"]] == g["trace"] and len(g["trace"]) == g["depth"]
    assert FIXTURE["pair7"]["oracle_agrees"] is True
    for entry, ref in (("parity_pair_actions", PARITY["parity_pair"]), ("c1_actions", PARITY["c1"]),
                       ("pair6_actions", SAFETY_FIXTURE["pair6_nocommit"]), ("safety_trio6_actions", SAFETY_FIXTURE["safety_trio6"])):
        g = FIXTURE[entry]
        assert g["verdict"] == "OK" and (g["generated"], g["distinct"], g["depth"], g["levels"]) == \
            (ref["generated"], ref["distinct"], ref["depth"], ref["levels"]), entry
    for entry in ("parity_pair_actions", "c1_actions"):
        assert {k: v[0] for k, v in FIXTURE[entry]["actions"].items()} == {k: v[0] for k, v in PARITY[FIXTURE[entry]["cfg"][:-8]]["actions"].items()}
    # the issue's scratch numbers, which the literal evaluator confirms
    a, b = FIXTURE["pair7_commit_regress"], FIXTURE["pair7_commit_regress_inmodel"]
    assert (a["verdict"], a["violated"], a["depth"], a["trace_actions"][-1]) == ("ACTION_PROPERTY_VIOLATION", FAILING, 19, "HandleAppendEntriesRequest")
    assert (b["verdict"], b["violated"], b["depth"]) == ("ACTION_PROPERTY_VIOLATION", FAILING, 21)
    assert FIXTURE["parity_pair_stepdown"]["violated"] == CONTROL


@pytest.mark.parametrize("entry", VIOLATED)
def test_counterexamples_are_behaviours(entry, tmp_path):
    """(d) The oracle's check-trace accepts each counterexample as a behaviour of the cfg without its
    PROPERTIES line, with no invariant violated.  check-trace asks every step to stay in the model, and with
    MC_COMPAT_INV_OUT_OF_MODEL the pair7 counterexample's last state is out of the model (handling the old request
    takes its count from 0 to -1, and the reply is a second copy of a response in the bag): it is replayed
    against the same cfg with message counts in -1..2 (WIDE_COUNTS), under which every earlier state is in the
    model too, and against the cfg itself the only step refused is that last one."""
    g = FIXTURE[entry]
    base = os.path.join(CONFIGS, "pair7.cfg" if entry.startswith("pair7") else "parity_pair.cfg")
    lines = g["trace"]
    if entry == "pair7_commit_regress":
        o = check_trace(base, lines, tmp_path, "exact.txt")
        assert o["bad_step"] == len(lines) - 1 and o["violated"] == "", o
        cfg = cfg_variant(base, replace=WIDE_COUNTS)
    else:
        cfg = cfg_variant(base)
    try:
        o = check_trace(cfg, lines, tmp_path)
    finally:
        os.unlink(cfg)
    assert o["bad_step"] == -1 and o["violated"] == "" and o["length"] == len(lines) == g["depth"], o
    assert o["actions"].split(",") == g["trace_actions"][1:], o
    if entry.startswith("pair7"):
        assert commit_regression(lines[-2], lines[-1]), lines[-2:]
        assert not any(commit_regression(a, b) for a, b in zip(lines[:-2], lines[1:-1]))
    else:   # the control: some leader of the last-but-one state is no leader in the last
        a, b = per_server(state_fields(lines[-2])["state"]), per_server(state_fields(lines[-1])["state"])
        assert any(a[s] == "Leader" and b[s] != "Leader" for s in a), lines[-2:]


# ---------------------------------------------------------------- (e) the boundary (mc_open only: no device)
def props_cfg(base, names, section="PROPERTIES"):
    return cfg_variant(os.path.join(CONFIGS, base + ".cfg"), append=section + "\n" + "".join("    %s\n" % n for n in names))


def test_names_open_through_the_wrapper(raftmc):
    for spec, section in ((ACTIONS_MC, "PROPERTIES"), (ACTIONS_SYM_MC, "PROPERTY")):
        cfg = props_cfg("c2", SIX, section)
        try:
            with raftmc.ModelChecker(spec, cfg) as mc:
                d = mc.describe()
        finally:
            os.unlink(cfg)
        assert d["properties"] == SIX and d["spec"] == "raft_original", d
    for name in ("pair7_commit_regress", "parity_pair_actions", "parity_pair_stepdown", "c1_actions", "pair6_actions", "safety_trio6_actions"):
        with raftmc.ModelChecker(ACTIONS_MC, os.path.join(CONFIGS, name + ".cfg")) as mc:
            assert mc.describe()["properties"], name


def test_description_without_properties_is_unchanged(raftmc):
    """A cfg without PROPERTIES keeps its description -- the checkpoint's model identity -- through the new
    wrapper: no "properties" key, and the text mc_describe gives through the plain wrapper."""
    texts = []
    for spec in (ORIG_MC, ACTIONS_MC):
        with raftmc.ModelChecker(spec, os.path.join(CONFIGS, "c2.cfg")) as mc:
            texts.append(mc._text(mc.lib.mc_describe))
    assert texts[0] == texts[1] and "properties" not in texts[0]


def test_pair7_shape_is_compiled(raftmc):
    with raftmc.ModelChecker(ORIG_MC, os.path.join(CONFIGS, "pair7.cfg")) as mc:
        d = mc.describe()
    assert (d["N"], d["NV"], d["MaxTerm"], d["MaxLogLen"], d["MaxMsgDomain"]) == (2, 1, 2, 1, 7), d


def refused(raftmc, spec, cfg):
    try:
        with pytest.raises(raftmc.RaftMCError) as e:
            raftmc.ModelChecker(spec, cfg)
    finally:
        os.unlink(cfg)
    assert e.value.code == -4, str(e.value)   # MC_E_UNSUPPORTED
    return str(e.value)


def test_plain_wrapper_refuses_the_names(raftmc):
    for name in SIX:
        msg = refused(raftmc, ORIG_MC, props_cfg("c2", [name]))
        assert name in msg and "raft_original_actions_mc.tla" in msg and "do not define" in msg, msg


def test_unknown_and_liveness_names_are_refused(raftmc):
    for name in ("TermsNeverGrow", "Liveness", "EventuallyLeader"):
        msg = refused(raftmc, ACTIONS_MC, props_cfg("c2", ["TermsMonotonic", name]))
        assert name in msg and "only the [][A]_vars properties" in msg, msg


def test_tlc_membership_stays_refused(raftmc):
    cfg = cfg_variant(os.path.join(CONFIGS, "memb_two.cfg"), append="PROPERTIES\n    TermsMonotonic\n")
    msg = refused(raftmc, os.path.join(CONFIGS, "raft_membership_mc.tla"), cfg)
    assert msg.endswith("temporal PROPERTIES are not supported"), msg
