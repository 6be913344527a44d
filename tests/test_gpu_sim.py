"""Simulation mode (TLC -simulate) on the GPU (MI355X): orig_simulate through the C ABI, the Python
mirror and the CLI, against the host mirror (tests/native/orig_sim_host.cpp, tests/test_sim_host.py)
bit for bit and against the CPU oracle's check-trace.  SMALL tables throughout: a simulation
allocates neither a seen-set nor a store."""
import json
import os
import subprocess

import pytest

from oracle_util import CONFIGS, GOLDEN, MEMB_MC, ORIG_MC
from test_sim_host import C2_SHAPE, PAIR_SHAPE, check_trace, pair_noleader_cfg, sim_host, sim_host_walk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raft-tla_amd", "_build", "raftmc")
SMALL = dict(fp_table_bytes=1 << 26, state_store_bytes=1 << 28)
WALKS = (0, 63, 64, 1023, 1024, 4095)   # a wave edge, a batch edge, the last walk


@pytest.fixture(scope="module")
def pair_cfg():
    path = pair_noleader_cfg()
    yield path
    os.unlink(path)


def trace_states(r):
    """(action, one-line state) per "State k:" block of a trace"""
    out = []
    for blk in r.trace_text.strip().split("\n\n"):
        head, *body = blk.split("\n")
        act = "Init" if "<Initial predicate>" in head else head.split("<", 1)[1].split(" ")[0].rstrip(">")
        out.append((act, " ".join(body)))
    return out


def summary_of(r):
    return (r.verdict, r.violated, r.generated, r.distinct, r.left_on_queue, r.depth, r.walks, r.steps, r.event_walk,
            {k: tuple(v) for k, v in r.actions.items()}, r.trace_text)


@pytest.fixture(scope="module")
def pair_election(raftmc, pair_cfg):
    """pair + NoLeader, seed 1, 4096 walks of depth 32 in one batch (test_sim_host's run), on the GPU."""
    with raftmc.ModelChecker(ORIG_MC, pair_cfg, seed=1, max_depth=32, **SMALL) as mc:
        return mc.simulate(4096, 4096)


@pytest.mark.parametrize("name", ["pair_noleader", "c2"])
def test_gpu_equals_host_bit_for_bit(raftmc, pair_cfg, name):
    """Seed 1, 4096 walks of depth 32 in batches of 1024, MC_COMPAT_INV_OUT_OF_MODEL cleared on both
    sides: generated, per-action generated counts, steps and walks equal the host mirror's (on
    pair + NoLeader both sides stop after the first batch, which holds an election), and the walks
    at a wave edge, a batch edge and the end are the mirror's line for line."""
    cfg, shape = (pair_cfg, PAIR_SHAPE) if name == "pair_noleader" else (os.path.join(CONFIGS, "c2.cfg"), C2_SHAPE)
    host = sim_host(shape, cfg, 1, 4096, 32, 1024, "--no-inv-oom")
    with raftmc.ModelChecker(ORIG_MC, cfg, seed=1, max_depth=32, inv_out_of_model=False, **SMALL) as mc:
        r = mc.simulate(4096, 1024)
        walks = {w: mc.sim_walk(w) for w in WALKS}
    print(name, "gpu", r.generated, r.steps, r.walks, r.event_walk, "host", host["generated"], host["steps"], host["walks"], host["event"])
    assert (r.generated, r.steps, r.walks, r.depth) == (host["generated"], host["steps"], host["walks"], host["depth"])
    assert {k: v[0] for k, v in r.actions.items()} == host["actions"]
    assert all(v[1] == 0 for v in r.actions.values())
    assert (r.distinct, r.left_on_queue, r.levels) == (0, 0, [])
    assert r.event_walk == (host["event"]["walk"] if host["event"] else -1)
    if name == "c2":
        assert r.verdict == "OK" and r.walks == 4096 and "collision" not in r.report and "calculated" not in r.report
    for w in WALKS:
        assert walks[w] == sim_host_walk(shape, cfg, 1, 32, w, "--no-inv-oom"), w


def test_same_inputs_same_result_other_seed_other_walk(raftmc):
    cfg = os.path.join(CONFIGS, "c2.cfg")
    runs = []
    for seed in (1, 1, 2):
        with raftmc.ModelChecker(ORIG_MC, cfg, seed=seed, max_depth=32, **SMALL) as mc:
            r = mc.simulate(4096, 1024)
            runs.append((summary_of(r), mc.sim_walk(5)))
    assert runs[0] == runs[1]
    assert runs[2][1] != runs[0][1]
    assert runs[2][0] != runs[0][0]


def test_election_found_on_the_pair_model(raftmc, pair_cfg, pair_election, tmp_path):
    """The run of test_sim_host's election test on the GPU: the same event (walk, trace length,
    states), printed as a BFS counterexample and valid for the oracle."""
    r = pair_election
    host = sim_host(PAIR_SHAPE, pair_cfg, 1, 4096, 32, 4096)
    assert r.verdict == "INVARIANT_VIOLATION" and r.violated == "NoLeader" and r.exit_code == 12, (r, r.error)
    assert host["event"] is not None
    states = [st for _, st in trace_states(r)]
    assert (r.event_walk, len(states)) == (host["event"]["walk"], host["event"]["length"])
    assert states == sim_host_walk(PAIR_SHAPE, pair_cfg, 1, 32, host["event"]["walk"])
    assert (r.generated, r.steps, r.walks) == (host["generated"], host["steps"], host["walks"])
    assert "<BecomeLeader" in r.trace_text.strip().split("\n\n")[-1].split("\n")[0]
    assert "Error: Invariant NoLeader is violated." in r.report
    o = check_trace(pair_cfg, states, tmp_path)
    assert o["valid"] and o["violated"] == "NoLeader" and o["length"] == len(states), o


def test_c5_election_without_a_table(raftmc, tmp_path):
    """The 5-server election that the BFS reaches at depth 14 behind 301.6M states (32 GB seen-set,
    112 GB store, test_gpu.py test_c5_compact_election_records) found by 2^20 random walks of depth
    64 with no table at all.  Seen on an MI355X: the first batch (262144 walks, 16.5M steps, 484M
    successors) already holds elections, 8 ms in the kernel, 0.02 s for the whole test call."""
    cfg = os.path.join(CONFIGS, "c5e_noleader.cfg")
    with raftmc.ModelChecker(ORIG_MC, cfg, seed=1, max_depth=64, **SMALL) as mc:
        r = mc.simulate(1 << 20)
    print("c5e_noleader: %d walks, %d steps, %d generated, %.3f s (%.3f s in the kernel), event walk %d, trace of %d states"
          % (r.walks, r.steps, r.generated, r.seconds, r.kernel_seconds, r.event_walk, r.depth))
    assert r.verdict == "INVARIANT_VIOLATION" and r.violated == "NoLeader" and r.exit_code == 12, (r, r.error)
    states = [st for _, st in trace_states(r)]
    assert len(states) >= 14
    assert "eleader" in states[-1]
    o = check_trace(cfg, states, tmp_path)
    assert o["valid"] and o["violated"] == "NoLeader" and o["length"] == len(states), o


def test_refusals(raftmc, tmp_path):
    """Simulation is raft_original's (hand-compiled), on one GPU, without checkpoints; the other
    families refuse it rather than run a BFS; a handle that never asked for it runs the BFS."""
    with raftmc.ModelChecker(MEMB_MC, os.path.join(CONFIGS, "memb_four.cfg"), **SMALL) as mc:
        with pytest.raises(raftmc.RaftMCError) as e:
            mc.simulate(1024)
        assert e.value.code == -4 and "raft_original" in str(e.value)
    ring = os.path.join(CONFIGS, "tlagen", "TokenRing.tla")
    with raftmc.ModelChecker(ring, os.path.join(CONFIGS, "tlagen", "TokenRing.cfg"), frontend="generated", workers=0, **SMALL) as mc:
        with pytest.raises(raftmc.RaftMCError) as e:
            mc.simulate(1024)
        assert e.value.code == -4
    pair = os.path.join(CONFIGS, "parity_pair.cfg")
    with raftmc.ModelChecker(ORIG_MC, pair, **SMALL) as mc:
        mc.set_checkpoint(str(tmp_path / "x.ckpt"), 1)
        with pytest.raises(raftmc.RaftMCError) as e:
            mc.simulate(1024)
        assert e.value.code == -4
    with raftmc.ModelChecker(ORIG_MC, pair, n_gpus=2, same_device=True, **SMALL) as mc:
        with pytest.raises(raftmc.RaftMCError):
            mc.simulate(1024)
    with raftmc.ModelChecker(ORIG_MC, pair, seed=1, max_depth=16, **SMALL) as mc:
        r = mc.simulate(1024)
        assert r.verdict == "OK" and r.walks == 1024
        with pytest.raises(raftmc.RaftMCError) as e:
            mc.dump_states(str(tmp_path / "dump.txt"))
        assert e.value.code == -7
        with pytest.raises(raftmc.RaftMCError):
            mc.collision_observed()
        with pytest.raises(raftmc.RaftMCError):
            mc.set_checkpoint(str(tmp_path / "y.ckpt"), 1)
    g = json.load(open(os.path.join(GOLDEN, "orig_parity.json")))["parity_pair"]
    with raftmc.ModelChecker(ORIG_MC, pair, **SMALL) as mc:
        r = mc.run()
    assert (r.verdict, r.generated, r.distinct, r.depth) == ("OK", g["generated"], g["distinct"], g["depth"])
    assert r.actions == g["actions"]


def test_cli_simulate(pair_cfg, pair_election):
    """raftmc -simulate num=4096 -depth 32 -seed 1: exit code 12, the trace of the Python run, and
    walks / steps on the -json line."""
    assert os.path.exists(CLI), "raftmc CLI not built"
    p = subprocess.run([CLI, "-simulate", "num=4096", "-depth", "32", "-seed", "1", "-json", "-config", pair_cfg, ORIG_MC],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 12, (p.stdout, p.stderr)
    assert "Error: Invariant NoLeader is violated." in p.stdout
    assert pair_election.trace_text in p.stdout
    js = json.loads(p.stdout.strip().splitlines()[-1])
    assert (js["walks"], js["steps"], js["generated"]) == (pair_election.walks, pair_election.steps, pair_election.generated)
    assert js["event_walk"] == pair_election.event_walk


def test_tlc_main_passes_simulate_through(raftmc, pair_cfg, pair_election, capsys):
    """The Python mirror of the command line: -simulate num=N -depth D -seed S reach simulate()."""
    code = raftmc.tlc_main(["-simulate", "num=4096", "-depth", "32", "-seed", "1", "-config", pair_cfg, ORIG_MC])
    out = capsys.readouterr().out
    assert code == 12
    assert "Error: Invariant NoLeader is violated." in out and pair_election.trace_text in out
    assert "%d walks of at most 32 states, %d steps, %d states generated." % (pair_election.walks, pair_election.steps,
                                                                             pair_election.generated) in out
    with pytest.raises(ValueError):
        raftmc.tlc_main(["-simulate", "-aril", "3", "-config", pair_cfg, ORIG_MC])
