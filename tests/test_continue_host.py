"""Continue mode (mc_set_continue) without a GPU: the host mirror of its rules
(tests/native/memb_witness_host.cpp, the product's packed spec in a FIFO BFS that keeps searching
after a violation) against the oracle-pinned single-property fixtures, and the refusals of the C ABI.

Invariants never decide which states are explored and a violating state is still enqueued, so the
search up to invariant X's first violation is the search of a plain run listing X: every witness
of a run over several scenario properties must equal the existing `scen_*` fixture of its property
(tests/golden/memb_parity.json), counters and state."""
import json
import os
import subprocess

import pytest

from oracle_util import CONFIGS, GOLDEN, MEMB_MC, ORIG_MC, ROOT, cfg_variant, native_build_dir

FIX = json.load(open(os.path.join(GOLDEN, "memb_parity.json")))


def build_mirror(shape=(3, 2)):
    out = os.path.join(native_build_dir(), "memb_witness_host_%d%d" % shape)
    csrc = os.path.join(ROOT, "raft-tla_amd", "csrc")
    src = [os.path.join(ROOT, "tests", "native", "memb_witness_host.cpp"), os.path.join(csrc, "model.cpp"),
           os.path.join(csrc, "memb_model.cpp"), os.path.join(csrc, "tla_value.cpp")]
    deps = src + [os.path.join(csrc, f) for f in ("memb_spec.h", "memb_text.h", "tla_value.h", "common.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in deps):
        tmp = "%s.%d" % (out, os.getpid())    # build aside and rename: parallel workers never run a partial file
        subprocess.run(["g++", "-O2", "-std=c++17", "-DSHAPE_N=%d" % shape[0], "-DSHAPE_NV=%d" % shape[1], "-o", tmp, *src],
                       check=True)
        os.replace(tmp, out)
    return out


def listing(base, props):
    """`base` (a scen_all_*.cfg) with only `props` under INVARIANTS, in that order; a temp path"""
    text = open(os.path.join(CONFIGS, base + ".cfg")).read()
    head = text[:text.index("INVARIANTS")]
    path = cfg_variant(os.path.join(CONFIGS, base + ".cfg"))
    with open(path, "w") as f:
        f.write(head + "INVARIANTS\n" + "".join("    %s\n" % p for p in props))
    return path


def mirror(cfg, tlc, max_depth=0):
    env = dict(os.environ, SYM_TLC="1") if tlc else None
    out = subprocess.run([build_mirror(), cfg, str(max_depth)], capture_output=True, text=True, check=True, env=env).stdout
    recs = [json.loads(l) for l in out.splitlines()]
    return recs[:-1], recs[-1]["summary"]


GROUPS = {"shipped": ("scen_all_shipped", ["EntryCommitted", "FirstBecomeLeader", "FirstCommit", "FirstRestart"], 16),
          "dynamic3": ("scen_all_dynamic3", ["AddSucessful", "MembershipChange", "MembershipChangeCommits"], 14)}


@pytest.mark.parametrize("tlc", [False, True], ids=["orbit", "tlc"])
@pytest.mark.parametrize("group", sorted(GROUPS))
def test_mirror_witnesses_equal_single_property_fixtures(group, tlc):
    base, props, deepest = GROUPS[group]
    cfg = listing(base, props)
    try:
        wits, summ = mirror(cfg, tlc)
    finally:
        os.unlink(cfg)
    assert summ["verdict"] == "OK" and summ["err"] == 0 and summ["pending"] == 0
    assert sorted(w["invariant"] for w in wits) == sorted(props)      # one witness per listed property
    for w in wits:
        g = FIX[("tlc:" if tlc else "") + "scen_" + w["invariant"]]
        assert g["depth"] <= deepest
        assert (w["depth"], w["generated"], w["distinct"], w["left_on_queue"]) == (g["depth"], g["generated"], g["distinct"], g["left_on_queue"]), w["invariant"]
        assert w["state"] == g["trace"][-1]["state"], w["invariant"]
        assert props[w["position"]] == w["invariant"]
    # discovery order: depth, then key (one state may be the witness of several: cfg position last)
    order = [(w["depth"], w["key"], w["position"]) for w in wits]
    assert order == sorted(order)
    # the run ends on the witness that empties the pending set: the last witness's stop point
    last = wits[-1]
    assert (summ["depth"], summ["generated"], summ["distinct"], summ["left_on_queue"]) == (
        last["depth"], last["generated"], last["distinct"], last["left_on_queue"])


def test_mirror_one_state_is_the_witness_of_two_properties():
    """FirstCommit and EntryCommitted first fail on the same successor of the shipped model."""
    cfg = listing("scen_all_shipped", ["FirstCommit", "EntryCommitted"])
    try:
        wits, _ = mirror(cfg, False)
    finally:
        os.unlink(cfg)
    assert [w["invariant"] for w in wits] == ["FirstCommit", "EntryCommitted"]
    assert wits[0]["key"] == wits[1]["key"] and wits[0]["state"] == wits[1]["state"]


def test_mirror_depth_limit_keeps_the_shallower_witnesses():
    base, props, _ = GROUPS["shipped"]
    cfg = listing(base, props)
    try:
        wits, summ = mirror(cfg, False, max_depth=14)
    finally:
        os.unlink(cfg)
    g = FIX["membership_shipped@14"]      # the same model: the plain search without a violation
    assert sorted(w["invariant"] for w in wits) == ["FirstBecomeLeader", "FirstRestart"]
    assert (summ["generated"], summ["distinct"], summ["depth"], summ["left_on_queue"]) == (g["generated"], g["distinct"], g["depth"], g["left_on_queue"])


def test_combined_cfgs_hold_the_models_of_the_files_they_combine():
    def model(name):
        t = open(os.path.join(CONFIGS, name + ".cfg")).read()
        return t[t.index("CONSTANTS"):t.index("INVARIANTS")], t[t.index("INVARIANTS"):].split()[1:]
    for allcfg, props in (("scen_all_shipped", ["BoundedTrace", "ConcurrentLeaders", "EntryCommitted", "FirstBecomeLeader", "FirstCommit",
                                                "FirstRestart", "LeadershipChange"]),
                          ("scen_all_dynamic3", ["AddCommits", "AddSucessful", "MembershipChange", "MembershipChangeCommits",
                                                 "MultipleMembershipChanges"]),
                          ("scen_all_grow2", ["MultipleMembershipChangesCommit", "LeaderChangesDuringConfChange"])):
        body, invs = model(allcfg)
        assert sorted(invs) == sorted(props)
        for p in props:
            assert model("scen_" + p)[0] == body, (allcfg, p)


# ---------------------------------------------------------------------------- the C ABI without a GPU
def test_set_continue_refused_on_raft_original(raftmc):
    with raftmc.ModelChecker(ORIG_MC, os.path.join(CONFIGS, "c1.cfg")) as mc:
        with pytest.raises(raftmc.RaftMCError) as e:
            mc.set_continue()
        assert e.value.code == -4 and "tlc_membership" in str(e.value)


def test_set_continue_refused_on_the_generated_path(raftmc):
    with raftmc.ModelChecker(os.path.join(CONFIGS, "tlagen", "Countdown.tla"), os.path.join(CONFIGS, "tlagen", "Countdown.cfg"),
                             frontend="generated") as mc:
        with pytest.raises(raftmc.RaftMCError) as e:
            mc.set_continue()
        assert e.value.code == -4


def test_set_continue_and_checkpoints_exclude_each_other(raftmc, tmp_path):
    cfg = os.path.join(CONFIGS, "scen_all_shipped.cfg")
    with raftmc.ModelChecker(MEMB_MC, cfg) as mc:
        mc.set_checkpoint(str(tmp_path / "a.ckpt"), 1)
        with pytest.raises(raftmc.RaftMCError) as e:
            mc.set_continue()
        assert e.value.code == -4
    with raftmc.ModelChecker(MEMB_MC, cfg) as mc:
        mc.set_recover(str(tmp_path / "a.ckpt"))
        with pytest.raises(raftmc.RaftMCError) as e:
            mc.set_continue()
        assert e.value.code == -4
    with raftmc.ModelChecker(MEMB_MC, cfg) as mc:
        mc.set_continue()
        for call in (lambda: mc.set_checkpoint(str(tmp_path / "a.ckpt"), 1), lambda: mc.set_recover(str(tmp_path / "a.ckpt"))):
            with pytest.raises(raftmc.RaftMCError) as e:
                call()
            assert e.value.code == -4
        mc.set_continue(False)
        mc.set_checkpoint(str(tmp_path / "a.ckpt"), 1)       # off again: the handle is a plain one


def test_set_continue_refused_with_several_gpus(raftmc):
    with raftmc.ModelChecker(MEMB_MC, os.path.join(CONFIGS, "scen_all_shipped.cfg"), n_gpus=2, same_device=True) as mc:
        with pytest.raises(raftmc.RaftMCError) as e:
            mc.set_continue()
        assert e.value.code == -4


def test_witness_calls_before_a_run(raftmc):
    import ctypes
    with raftmc.ModelChecker(MEMB_MC, os.path.join(CONFIGS, "scen_all_shipped.cfg")) as mc:
        mc.set_continue()
        n = ctypes.c_int32()
        assert mc.lib.mc_witness_count(mc.h, ctypes.byref(n)) == -7
        w = raftmc.raftmc.McWitness()
        assert mc.lib.mc_witness(mc.h, 0, ctypes.byref(w), None, None) == -7
        assert mc.witnesses() == []


def test_witness_struct_layout_matches_ctypes_mirror(raftmc, tmp_path):
    """mc_witness_t as the C compiler lays it out: fixed size, a reserved tail"""
    import ctypes
    M = raftmc.raftmc.McWitness
    fields = [f[0] for f in M._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "raftmc.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(mc_witness_t));\n' +
                   "".join('  printf(" %%zu", offsetof(mc_witness_t, %s));\n' % f for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(M)] + [getattr(M, f).offset for f in fields]
    assert fields[-1] == "reserved"


def test_cli_accepts_continue():
    """-continue reaches mc_set_continue: raft_original is refused by name (exit 75), the membership cfg
    gets as far as the run (which needs a device)."""
    exe = os.path.join(ROOT, "raft-tla_amd", "_build", "raftmc")
    r = subprocess.run([exe, "-continue", "-config", os.path.join(CONFIGS, "c1.cfg"), ORIG_MC], capture_output=True, text=True)
    assert r.returncode == 75 and "continue mode" in r.stderr and "unknown option" not in r.stderr
    r = subprocess.run([exe, "-continue", "-gpus", "2", "-config", os.path.join(CONFIGS, "scen_all_shipped.cfg"), MEMB_MC],
                       capture_output=True, text=True)
    assert r.returncode == 75 and "one GPU" in r.stderr


def test_tlc_main_passes_continue_through(raftmc):
    with pytest.raises(raftmc.RaftMCError) as e:
        raftmc.tlc_main(["-continue", "-config", os.path.join(CONFIGS, "c1.cfg"), ORIG_MC])
    assert e.value.code == -4 and "continue mode" in str(e.value)
