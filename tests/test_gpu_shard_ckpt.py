"""Checkpoint and recover of multi-GPU raft_original runs, at any GPU count.

mc_run with mc_opts.n_gpus > 1 honours mc_set_checkpoint (a manifest and one file per rank,
path.g<levels>.r<rank>) and mc_set_recover, and a recovery takes a file written at another GPU count:
every stored state is fingerprinted again, placed with its new owner and its parent pointer
rewritten (csrc/orig_reshard.hip).  A search cut on W GPUs and finished on W' must give the
uninterrupted run's counts, levels, state set and a valid counterexample.  On a one-GPU machine the
ranks share cuda:0 (same_device), as in test_gpu_shard.py."""
import glob
import hashlib
import json
import os
import subprocess

import pytest
import torch

from oracle_util import CONFIGS, GOLDEN, MEMB_MC, ORIG_MC
from test_gpu_sim import trace_states
from test_sim_host import check_trace

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raft-tla_amd", "_build", "raftmc")
SMALL = dict(fp_table_bytes=1 << 26, state_store_bytes=1 << 28)
FIXTURES = json.load(open(os.path.join(GOLDEN, "orig_parity.json")))


def cfg_of(name):
    return os.path.join(CONFIGS, name + ".cfg")


def open_world(raftmc, cfg, world, **kw):
    """a handle of `world` GPUs; world 1 is a plain single-GPU -workers N handle"""
    kw = {**SMALL, **kw}
    if world == 1:
        return raftmc.ModelChecker(ORIG_MC, cfg, **{"workers": 0, **kw})
    return raftmc.ModelChecker(ORIG_MC, cfg, n_gpus=world, same_device=torch.cuda.device_count() < world, **kw)


def dump_lines(mc, world, tmp_path):
    """every stored state of the last run, one line each: path (one GPU) or path.rank<r>"""
    path = str(tmp_path / "dump.txt")
    mc.dump_states(path)
    files = [path] if world == 1 else ["%s.rank%d" % (path, r) for r in range(world)]
    lines = []
    for f in files:
        lines += [l.rstrip("\n") for l in open(f)]
        os.unlink(f)
    return lines


def states_sha(lines):
    return hashlib.sha256("\n".join(sorted(lines)).encode()).hexdigest()   # as tests/test_gpu.py states_sha


def generation_files(ck):
    return sorted(p for p in glob.glob(ck + "*") if p != ck)


def manifest_generation(ck):
    """the `generation` word of the manifest's header (csrc/ckpt_file.h ShardHead)"""
    head = open(ck, "rb").read(136)
    assert head[:8] == b"RAFTMCS1"
    return int.from_bytes(head[128:136], "little", signed=True)


def write_cut(raftmc, name, world, depth, ck, **kw):
    with open_world(raftmc, cfg_of(name), world, max_depth=depth, **kw) as mc:
        mc.set_checkpoint(ck, 1)
        r = mc.run()
    assert r.verdict == "DEPTH_LIMIT" and r.depth == depth, r.error
    return r


def assert_fixture(r, g):
    assert (r.verdict, r.generated, r.distinct, r.depth) == ("OK", g["generated"], g["distinct"], g["depth"]), r.error
    assert {k: v[0] for k, v in r.actions.items()} == {k: v[0] for k, v in g["actions"].items()}
    assert [lv[0] for lv in r.levels] == g["levels"]


def recover_to_end(raftmc, name, world, ck, tmp_path, **kw):
    g = FIXTURES[name]
    with open_world(raftmc, cfg_of(name), world, **kw) as mc:
        mc.set_recover(ck)
        r = mc.run()
        lines = dump_lines(mc, world, tmp_path)
    assert_fixture(r, g)
    assert len(lines) == g["distinct"] and states_sha(lines) == g["states_sha256"]
    return r


def test_same_world(raftmc, tmp_path):
    """c1 on 2 GPUs, a checkpoint behind every level to depth 6: the manifest and exactly the last
    generation's two rank files are left; 2 fresh GPUs finish the search from it."""
    ck = str(tmp_path / "c1.ckpt")
    write_cut(raftmc, "c1", 2, 6, ck)
    assert manifest_generation(ck) == 6
    assert generation_files(ck) == [ck + ".g6.r0", ck + ".g6.r1"]          # no .tmp, no older generation
    r = recover_to_end(raftmc, "c1", 2, ck, tmp_path)
    assert {"orig_reshard_classify", "orig_reshard_place", "orig_reinsert"} <= set(r.kernels)
    assert r.kernels["orig_reshard_classify"]["launches"] >= 6 and r.kernels["orig_reshard_place"]["launches"] >= 6


@pytest.mark.parametrize("name,world,new_world", [("c1", 1, 2), ("c1", 2, 1), ("c1", 2, 3), ("parity_pair_neg", 3, 2), ("parity_trio", 1, 3)])
def test_any_world_to_any_world(raftmc, tmp_path, name, world, new_world):
    """Cut at half the fixture's depth on `world` GPUs (1: a plain single-GPU -workers N checkpoint),
    finished on `new_world` (1: a plain single-GPU handle): the fixture's counts, per-action
    generated counts, level sizes and state set."""
    ck = str(tmp_path / "cut.ckpt")
    write_cut(raftmc, name, world, FIXTURES[name]["depth"] // 2, ck)
    recover_to_end(raftmc, name, new_world, ck, tmp_path)


def test_fifo_single_gpu_checkpoint_on_two_gpus(raftmc, tmp_path):
    """A single-GPU -workers 1 (FIFO order) checkpoint resumes a multi-GPU search too."""
    g = FIXTURES["c1"]
    ck = str(tmp_path / "fifo.ckpt")
    write_cut(raftmc, "c1", 1, 6, ck, workers=1)
    with open_world(raftmc, cfg_of("c1"), 2) as mc:
        mc.set_recover(ck)
        r = mc.run()
    assert (r.verdict, r.generated, r.distinct, r.depth) == ("OK", g["generated"], g["distinct"], g["depth"]), r.error


@pytest.mark.parametrize("world,new_world", [(2, 3), (1, 2), (2, 1)])
def test_parent_pointers_survive(raftmc, tmp_path, world, new_world):
    """scenario_first_leader (NoLeader at depth 10) cut at depth 6: the counterexample found after
    the recovery is chased through rewritten parent pointers, across the recovered levels, and the
    oracle accepts it."""
    cfg = cfg_of("scenario_first_leader")
    ck = str(tmp_path / "fl.ckpt")
    with open_world(raftmc, cfg, world, max_depth=6) as mc:
        mc.set_checkpoint(ck, 1)
        assert mc.run().verdict == "DEPTH_LIMIT"
    with open_world(raftmc, cfg, new_world) as mc:
        mc.set_recover(ck)
        r = mc.run()
    assert r.verdict == "INVARIANT_VIOLATION" and r.violated == "NoLeader" and r.exit_code == 12, r.error
    states = [st for _, st in trace_states(r)]
    assert len(states) == 10
    o = check_trace(cfg, states, tmp_path)
    assert o["valid"] and o["violated"] == "NoLeader" and o["length"] == 10, o


def _slot_bytes(raftmc, cfg):
    with raftmc.ModelChecker(ORIG_MC, cfg) as mc:
        return mc.describe()["state_bytes_stored"] + 8


def test_out_of_room_goes_on_with_more_ranks(raftmc, tmp_path):
    """parity_pair_big (569,162 states) on 2 GPUs whose stores hold 150,000 states each ends as
    CAPACITY_OVERFLOW; its last checkpoint is the last completed level.  3 GPUs finish it; 2 GPUs with
    the same small stores overflow again, at once and without a fault."""
    name = "parity_pair_big"
    g = FIXTURES[name]
    cfg = cfg_of(name)
    ck = str(tmp_path / "big.ckpt")
    tight = dict(state_store_bytes=150_000 * _slot_bytes(raftmc, cfg))
    with open_world(raftmc, cfg, 2, workers=0, **tight) as mc:
        mc.set_checkpoint(ck, 1)
        a = mc.run()
    assert a.verdict == "CAPACITY_OVERFLOW", a.error
    assert 2 < a.depth < g["depth"] and a.distinct == sum(g["levels"][:a.depth])
    assert manifest_generation(ck) == a.depth              # the levels the summary reports as completed
    assert generation_files(ck) == ["%s.g%d.r%d" % (ck, a.depth, k) for k in range(2)]
    with open_world(raftmc, cfg, 3) as mc:
        mc.set_recover(ck)
        assert_fixture(mc.run(), g)
    with open_world(raftmc, cfg, 2, **tight) as mc:
        mc.set_recover(ck)
        b = mc.run()
    assert b.verdict == "CAPACITY_OVERFLOW", (b.verdict, b.error)     # (its shares fit as they did; the next levels do not)
    assert a.depth <= b.depth < g["depth"] and b.distinct == sum(g["levels"][:b.depth])
    # a checkpoint that does not even fit: every rank's share is cut at its store's end
    with open_world(raftmc, cfg, 2, state_store_bytes=20_000 * _slot_bytes(raftmc, cfg)) as mc:
        mc.set_recover(ck)
        c = mc.run()
    assert c.verdict == "CAPACITY_OVERFLOW" and "state store full" in c.error, (c.verdict, c.error)
    assert (c.distinct, c.depth) == (a.distinct, a.depth)
    with open_world(raftmc, cfg, 1, state_store_bytes=20_000 * _slot_bytes(raftmc, cfg)) as mc:   # ... on one GPU too (no host spill here)
        mc.set_recover(ck)
        d = mc.run()
    assert d.verdict == "CAPACITY_OVERFLOW" and "state store full" in d.error, (d.verdict, d.error)


@pytest.mark.timeout(600)
def test_many_blocks_and_workgroups(raftmc, tmp_path):
    """c5v2 cut at depth 9 on 2 GPUs: the last level (2,648,995 states) spans three 2^20-state staging
    blocks and thousands of workgroups per block.  3 GPUs take it to depth 10: the single-GPU run's
    counts, per-action generated counts and level sizes.  (Tens of seconds: a 270 MB checkpoint.)"""
    cfg = cfg_of("c5v2")
    big = dict(fp_table_bytes=1 << 30, state_store_bytes=1 << 30)
    a = raftmc.check(ORIG_MC, cfg, max_depth=10, workers=0)
    assert a.verdict == "DEPTH_LIMIT" and a.distinct == 17_554_243
    assert [lv[0] for lv in a.levels][:9] == [1, 6, 45, 330, 2190, 13761, 82510, 475485, 2648995]
    ck = str(tmp_path / "c5.ckpt")
    with open_world(raftmc, cfg, 2, max_depth=9, workers=0, **big) as mc:
        mc.set_checkpoint(ck, 9)
        assert mc.run().verdict == "DEPTH_LIMIT"
    assert manifest_generation(ck) == 9
    with open_world(raftmc, cfg, 3, max_depth=10, workers=0, **big) as mc:
        mc.set_recover(ck)
        r = mc.run()
    assert (r.verdict, r.generated, r.distinct, r.depth, r.left_on_queue) == ("DEPTH_LIMIT", a.generated, a.distinct, a.depth, a.left_on_queue), r.error
    assert {k: v[0] for k, v in r.actions.items()} == {k: v[0] for k, v in a.actions.items()}
    assert [lv[0] for lv in r.levels] == [lv[0] for lv in a.levels]


def test_refusals_that_stay(raftmc, tmp_path):
    import ctypes
    ck = str(tmp_path / "r.ckpt")
    # tlc_membership on 2 GPUs with a checkpoint: refused at run(), the family named
    with raftmc.ModelChecker(MEMB_MC, cfg_of("membership_shipped"), n_gpus=2, same_device=torch.cuda.device_count() < 2, **SMALL) as mc:
        mc.set_checkpoint(ck, 1)
        with pytest.raises(raftmc.RaftMCError) as e:
            mc.run()
    assert e.value.code == -4 and "tlc_membership" in str(e.value)
    assert not os.path.exists(ck)
    # the step API on a checkpointing handle
    with raftmc.ModelChecker(ORIG_MC, cfg_of("c1")) as mc:
        mc.set_checkpoint(ck, 1)
        mc.lib.mc_shard_open.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32]
        assert mc.lib.mc_shard_open(mc.h, 0, 2) == -4
    write_cut(raftmc, "c1", 2, 6, ck)
    # a multi-GPU checkpoint is a -workers N one
    with raftmc.ModelChecker(ORIG_MC, cfg_of("c1"), workers=1, **SMALL) as mc:
        mc.set_recover(ck)
        with pytest.raises(raftmc.RaftMCError) as e:
            mc.run()
    assert e.value.code == -1 and "-workers N" in str(e.value)
    # ... of its own model
    for world in (1, 2):
        with open_world(raftmc, cfg_of("parity_pair"), world) as mc:
            mc.set_recover(ck)
            with pytest.raises(raftmc.RaftMCError) as e:
                mc.run()
        assert e.value.code == -1, world
    # a rank file cut to half its length: the I/O error; deleted: no checkpoint
    rank1 = ck + ".g6.r1"
    whole = open(rank1, "rb").read()
    open(rank1, "wb").write(whole[:len(whole) // 2])
    for world in (1, 3):
        with open_world(raftmc, cfg_of("c1"), world) as mc:
            mc.set_recover(ck)
            with pytest.raises(raftmc.RaftMCError) as e:
                mc.run()
        assert e.value.code == -2 and "truncated" in str(e.value), (world, str(e.value))
    os.unlink(rank1)
    for world in (1, 2):
        with open_world(raftmc, cfg_of("c1"), world) as mc:
            mc.set_recover(ck)
            with pytest.raises(raftmc.RaftMCError) as e:
                mc.run()
        assert e.value.code == -1 and "missing" in str(e.value), (world, str(e.value))


def test_cli_checkpoint_and_recover_on_two_gpus(tmp_path):
    """raftmc -gpus 2 -checkpoint 1 -depth 6 on c1, then -recover: exit code 0 and TLC's summary
    lines with the fixture's counts.  -same-device puts both ranks on one GPU where there is only one."""
    g = FIXTURES["c1"]
    ck = str(tmp_path / "cli.ckpt")
    common = ["-gpus", "2", "-config", cfg_of("c1"), "-fptable", str(1 << 26), "-store", str(1 << 28)]
    if torch.cuda.device_count() < 2:
        common.append("-same-device")
    a = subprocess.run([CLI, *common, "-checkpoint", "1", "-checkpoint-file", ck, "-depth", "6", ORIG_MC], capture_output=True, text=True, timeout=300)
    assert a.returncode == 0 and "Verdict: DEPTH_LIMIT" in a.stdout, a.stderr
    assert os.path.exists(ck) and generation_files(ck) == [ck + ".g6.r0", ck + ".g6.r1"]
    b = subprocess.run([CLI, *common, "-recover", ck, ORIG_MC], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    assert "%d states generated, %d distinct states found, 0 states left on queue." % (g["generated"], g["distinct"]) in b.stdout
    assert "The depth of the complete state graph search is %d." % g["depth"] in b.stdout


def test_read_state_after_release(raftmc):
    """mc_shard_read_state (which the multi-GPU trace chase calls) on a handle whose device memory was
    released: MC_E_STATE, not a copy from a store that is gone."""
    import ctypes
    with raftmc.ModelChecker(ORIG_MC, cfg_of("c1"), **SMALL) as mc:
        lib = mc.lib
        lib.mc_shard_open.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32]
        lib.mc_shard_read_state.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_void_p),
                                            ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_uint64)]
        assert lib.mc_shard_open(mc.h, 0, 1) == 0
        text, n, meta = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_uint64()
        assert lib.mc_shard_read_state(mc.h, 0, ctypes.byref(text), ctypes.byref(n), ctypes.byref(meta)) == 0
        assert meta.value == (1 << 64) - 1 and b"currentTerm" in ctypes.string_at(text, n.value)
        lib.mc_free(text)
        mc.release_device_memory()
        assert lib.mc_shard_read_state(mc.h, 0, ctypes.byref(text), ctypes.byref(n), ctypes.byref(meta)) == -7
        assert b"released" in lib.mc_last_error(mc.h)
