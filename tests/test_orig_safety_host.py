"""Raft's log- and commit-safety invariants on raft_original (configs/raft_original_safety_mc.tla,
DESIGN.md §12) on the host (no GPU): the packed evaluation the kernels compile (csrc/orig_spec.h
violated_safety, inv_frame_safety) against a literal evaluator of each definition
(tests/native/orig_safety_host.cpp), the boundary (mc_open), and tests/golden/orig_safety.json
(written by tests/golden/make_orig_safety.py from the generated front end's host BFS, a second
implementation compiled from the unmodified reference text) reproduced by the generated path."""
import json
import os
import subprocess
import tempfile

import pytest

from oracle_util import CONFIGS, GOLDEN, ORIG_MC, ROOT, cfg_variant, native_build_dir
from test_tlagen import needs_ref, needs_tool

SAFETY_MC = os.path.join(CONFIGS, "raft_original_safety_mc.tla")
FIXTURE = json.load(open(os.path.join(GOLDEN, "orig_safety.json")))
SAFETY = ["CommitWithinLog", "LeaderVotesQuorum", "CandidateTermNotInLog", "LeaderHasLatestOfTerm", "VotesGrantedInv",
          "QuorumLogInv", "MoreUpToDateCorrect", "LeaderCompleteness", "StateMachineSafety"]
CONTROL = "AllHaveCommitted_false"
ELEVEN = ["ElectionSafety", "LogMatching"] + SAFETY
# (N, NV, MaxTerm, MaxLogLen, MaxMsgDomain) of each cfg
SHAPES = {"parity_pair": (2, 1, 2, 1, 5), "pair6_nocommit": (2, 1, 2, 1, 6), "c1": (3, 1, 2, 1, 2), "safety_trio6": (3, 1, 2, 1, 6)}
# mutated copies per reachable state (seeded): enough for every invariant to fail somewhere (below)
MUTATIONS = 8


def safety_cfg(name, invariants, append=""):
    """configs/<name>.cfg with its INVARIANTS section (the last one of these cfgs) replaced (a temp
    file; the caller unlinks it)"""
    text = open(os.path.join(CONFIGS, name + ".cfg")).read()
    head, sep, _ = text.partition("INVARIANTS\n")
    assert sep, name
    fd, path = tempfile.mkstemp(suffix=".cfg")
    with os.fdopen(fd, "w") as f:
        f.write(head + "INVARIANTS\n" + "".join("    %s\n" % n for n in invariants) + append)
    return path


def build_safety_host(shape):
    """Compile tests/native/orig_safety_host.cpp for one shape (as test_orig_symmetry_host builds its harness)."""
    out = os.path.join(native_build_dir(), "orig_safety_host_%d%d%d%d%d" % shape)
    csrc = os.path.join(ROOT, "raft-tla_amd", "csrc")
    src = [os.path.join(ROOT, "tests", "native", "orig_safety_host.cpp"), os.path.join(csrc, "model.cpp"), os.path.join(csrc, "orig_model.cpp")]
    deps = src + [os.path.join(csrc, h) for h in ("orig_spec.h", "orig_text.h", "common.h", "model.h")]
    if os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps):
        return out
    tmp = "%s.%d" % (out, os.getpid())
    subprocess.run(["g++", "-O2", "-std=c++17", "-DSHAPE_N=%d" % shape[0], "-DSHAPE_NV=%d" % shape[1], "-DSHAPE_MT=%d" % shape[2],
                    "-DSHAPE_ML=%d" % shape[3], "-DSHAPE_MK=%d" % shape[4], "-o", tmp, *src], check=True)
    os.replace(tmp, out)
    return out


@pytest.fixture(scope="module")
def host_checks():
    """name -> the harness's report over the model's whole reachable set, computed once"""
    out = {}
    for name in ("parity_pair", "pair6_nocommit", "c1"):
        r = subprocess.run([build_safety_host(SHAPES[name]), os.path.join(CONFIGS, name + ".cfg"), "--mutations", str(MUTATIONS), "--seed", "1"],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        out[name] = json.loads(r.stdout.strip().splitlines()[-1])
    return out


def test_packed_evaluation_equals_the_literal_definitions(host_checks):
    """Every reachable state, every out-of-model successor and MUTATIONS mutated copies of every
    reachable state of the three models: WithSafety<S>::violated equals the literal evaluator bit for
    bit, and each of the nine invariants and the control is false somewhere and true somewhere
    (QuorumLogInv cannot fail with two servers -- a server holds its own committed prefix and is half
    of Server -- so the condition is over the three models together).
    Measured with MUTATIONS = 8, seed 1: [true, false] per invariant are printed by the harness."""
    states = {"parity_pair": 20938, "pair6_nocommit": 85322, "c1": 3304}   # tests/golden/orig_safety.json
    total = {n: [0, 0] for n in SAFETY + [CONTROL]}
    for name, c in host_checks.items():
        print(name, json.dumps(c))
        assert c["states"] == states[name] == FIXTURE[name]["distinct"], c
        assert c["compared"] > (1 + MUTATIONS) * c["states"] and c["disagreements"] == 0, c
        for n, (t, f) in c["invariants"].items():
            total[n][0] += t
            total[n][1] += f
    assert sorted(total) == sorted(SAFETY + [CONTROL])
    assert all(t > 0 and f > 0 for t, f in total.values()), total


def test_frame_conditions_hold_on_every_reachable_transition(host_checks):
    """inv_frame: on every reachable (state, successor, action), in or out of the model, an invariant
    (the two old ones, the nine and the control) that holds in the parent and fails in the successor is
    one the action's frame names -- so evaluating only inv_frame(action) on a successor loses nothing."""
    generated = {"parity_pair": 408109, "pair6_nocommit": 1906605, "c1": 50740}
    for name, c in host_checks.items():
        assert c["frame_checked"] == generated[name] - 1 and c["frame_bad"] == 0, (name, c)


# ---------------------------------------------------------------- the boundary (mc_open only: no device)
def test_names_open_through_the_wrapper(raftmc):
    cfg = safety_cfg("c2", ELEVEN + [CONTROL])
    try:
        with raftmc.ModelChecker(SAFETY_MC, cfg) as mc:
            d = mc.describe()
    finally:
        os.unlink(cfg)
    assert d["invariants"] == ELEVEN + [CONTROL] and d["spec"] == "raft_original", d


def test_plain_wrapper_refuses_the_names(raftmc):
    for name in SAFETY + [CONTROL]:
        cfg = safety_cfg("c2", ["ElectionSafety", name])
        try:
            with pytest.raises(raftmc.RaftMCError) as e:
                raftmc.ModelChecker(ORIG_MC, cfg)
        finally:
            os.unlink(cfg)
        assert e.value.code == -4 and name in str(e.value) and "raft_original_safety_mc.tla" in str(e.value), str(e.value)


def test_unknown_names_stay_unknown(raftmc):
    cfg = safety_cfg("c2", ["ElectionSafety", "VotesGrantedInv_false"])
    try:
        with pytest.raises(raftmc.RaftMCError) as e:
            raftmc.ModelChecker(SAFETY_MC, cfg)
    finally:
        os.unlink(cfg)
    assert e.value.code == -4 and "unknown invariant 'VotesGrantedInv_false'" in str(e.value), str(e.value)


def test_description_without_the_names_is_unchanged(raftmc):
    """A cfg that lists none of the new names keeps its description -- the checkpoint's model identity
    -- byte for byte, through either wrapper: C2's, as the library printed it before the names existed."""
    want = ('{"spec": "raft_original", "N": 3, "NV": 2, "MaxTerm": 3, "MaxLogLen": 2, "MaxMsgDomain": 5, "MinMsgCount": 0, '
            '"MaxMsgCount": 1, "state_bits": 461, "state_words": 15, "state_bytes_stored": 64, "instances": 51, '
            '"log_universe": 43, "constraints": ["BoundedTerms", "BoundedLogs", "BoundedMessages"], '
            '"invariants": ["ElectionSafety", "LogMatching"], "actions": ["Restart", "Timeout", "RequestVote", "BecomeLeader", '
            '"ClientRequest", "AdvanceCommitIndex", "AppendEntries", "UpdateTerm", "HandleRequestVoteRequest", '
            '"DropStaleResponse", "HandleRequestVoteResponse", "HandleAppendEntriesRequest", '
            '"HandleAppendEntriesResponse", "DuplicateMessage", "DropMessage"], "symmetry_mode": "tlc", "workers": 1, '
            '"check_deadlock": true, "n_gpus": 1}')
    for spec in (ORIG_MC, SAFETY_MC):
        with raftmc.ModelChecker(spec, os.path.join(CONFIGS, "c2.cfg")) as mc:
            assert mc._text(mc.lib.mc_describe) == want


def test_safety_trio6_shape_is_compiled(raftmc):
    with raftmc.ModelChecker(ORIG_MC, os.path.join(CONFIGS, "safety_trio6.cfg")) as mc:
        d = mc.describe()
    assert (d["N"], d["NV"], d["MaxTerm"], d["MaxLogLen"], d["MaxMsgDomain"]) == SHAPES["safety_trio6"], d


@needs_tool
@needs_ref
@pytest.mark.parametrize("name", ["c1", "parity_pair"])
def test_fixture_reproduced_by_generated_path(name):
    from test_tlagen import generate, host_bfs
    g = FIXTURE[name]
    assert g["invariants"] == ELEVEN
    cfg = safety_cfg(g["cfg"], g["invariants"])
    try:
        r = host_bfs(generate(SAFETY_MC, cfg))
    finally:
        os.unlink(cfg)
    assert r["verdict"] == g["verdict"] == "OK" and r["err"] == 0
    assert (r["generated"], r["distinct"], r["depth"], r["levels"]) == (g["generated"], g["distinct"], g["depth"], g["levels"])
