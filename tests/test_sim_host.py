"""Simulation mode (TLC -simulate) on the host: tests/native/orig_sim_host.cpp, the single-threaded
mirror of the GPU walker over the product's successor function (csrc/orig_spec.h) and its
counter-based random numbers (csrc/sim_rng.h), validated by the CPU oracle's check-trace.  No GPU."""
import json
import os
import subprocess

import pytest

from oracle_util import CONFIGS, ORIG_MC, ROOT, cfg_variant, native_build_dir, run_oracle

PAIR_SHAPE = (2, 1, 2, 1, 5)
C2_SHAPE = (3, 2, 3, 2, 5)


def build_sim_host(shape):
    """Compile tests/native/orig_sim_host.cpp for one shape (as test_packed_semantics builds orig_walk.cpp)."""
    out = os.path.join(native_build_dir(), "orig_sim_host_%d%d%d%d%d" % shape)
    src = [os.path.join(ROOT, "tests", "native", "orig_sim_host.cpp"), os.path.join(ROOT, "raft-tla_amd", "csrc", "model.cpp"),
           os.path.join(ROOT, "raft-tla_amd", "csrc", "orig_model.cpp")]
    deps = src + [os.path.join(ROOT, "raft-tla_amd", "csrc", h) for h in ("orig_spec.h", "orig_text.h", "sim_rng.h", "common.h")]
    if os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps):
        return out
    tmp = "%s.%d" % (out, os.getpid())
    subprocess.run(["g++", "-O2", "-std=c++17", "-DSHAPE_N=%d" % shape[0], "-DSHAPE_NV=%d" % shape[1], "-DSHAPE_MT=%d" % shape[2],
                    "-DSHAPE_ML=%d" % shape[3], "-DSHAPE_MK=%d" % shape[4], "-o", tmp, *src], check=True)
    os.replace(tmp, out)
    return out


def sim_host(shape, cfg, seed, num, depth, batch, *extra):
    """The mirror's summary (JSON) for walks 0..num-1."""
    out = subprocess.run([build_sim_host(shape), cfg, str(seed), str(num), str(depth), str(batch), *extra],
                         capture_output=True, text=True, check=True, timeout=600).stdout
    return json.loads(out.strip().splitlines()[-1])


def sim_host_walk(shape, cfg, seed, depth, walk, *extra):
    """One walk of the mirror: its canonical state lines."""
    out = subprocess.run([build_sim_host(shape), cfg, str(seed), "1", str(depth), "1", "--walk", str(walk), *extra],
                         capture_output=True, text=True, check=True, timeout=600).stdout
    return out.strip().split("\n")


def pair_noleader_cfg():
    """parity_pair.cfg with NoLeader added to its invariants (a temp file)."""
    return cfg_variant(os.path.join(CONFIGS, "parity_pair.cfg"), replace=[("    LogMatching", "    LogMatching\n    NoLeader")])


def check_trace(cfg, lines, tmp_path, name="walk.txt"):
    p = tmp_path / name
    p.write_text("\n".join(lines) + "\n")
    return run_oracle("check-trace", ORIG_MC, cfg, "--golden", str(p))


@pytest.fixture(scope="module")
def pair_cfg():
    path = pair_noleader_cfg()
    yield path
    os.unlink(path)


@pytest.fixture(scope="module")
def pair_run(pair_cfg):
    """pair + NoLeader, seed 1, 4096 walks of depth 32 in one batch: shared by the tests below."""
    return sim_host(PAIR_SHAPE, pair_cfg, 1, 4096, 32, 4096)


def test_host_walks_are_valid_behaviours(tmp_path):
    """Walks of c2.cfg replayed by the oracle: Init is right, every step is an in-model successor of
    the literal restatement of raft_original.tla, no invariant is broken along the way."""
    cfg = os.path.join(CONFIGS, "c2.cfg")
    summary = sim_host(C2_SHAPE, cfg, 1, 256, 32, 256)
    assert summary["event"] is None and summary["walks"] == 256
    assert summary["generated"] == sum(summary["actions"].values())
    for w in (0, 1, 17, 255):
        lines = sim_host_walk(C2_SHAPE, cfg, 1, 32, w)
        assert 1 < len(lines) <= 32
        r = check_trace(cfg, lines, tmp_path, "walk%d.txt" % w)
        assert r["bad_step"] == -1 and r["violated"] == "" and r["length"] == len(lines), (w, r)


def test_host_mirror_finds_an_election_on_the_pair_model(pair_cfg, pair_run, tmp_path):
    """4096 uniform walks of depth 32 hold about 100 elections (99, 101, 110 over three seeds): the
    batch's event exists, its walk is a valid NoLeader counterexample for the oracle, and it is no
    shorter than the oracle's own BFS counterexample (the shortest one)."""
    ev = pair_run["event"]
    assert ev is not None, pair_run
    assert pair_run["actions"]["BecomeLeader"] >= 1
    lines = sim_host_walk(PAIR_SHAPE, pair_cfg, 1, 32, ev["walk"])
    assert len(lines) == ev["length"]
    r = check_trace(pair_cfg, lines, tmp_path)
    assert r["valid"] and r["violated"] == "NoLeader" and r["length"] == len(lines), r
    bfs = run_oracle("bfs", ORIG_MC, pair_cfg)
    assert bfs["verdict"] == "INVARIANT_VIOLATION" and bfs["violated"] == "NoLeader", bfs
    assert bfs["trace_len"] >= 2 and ev["length"] >= bfs["trace_len"], (ev, bfs["trace_len"])


def test_first_step_is_uniform(pair_run):
    """Init of the pair model has four enabled in-model instances (Restart(s1), Restart(s2), which
    reproduce Init, and Timeout(s1), Timeout(s2)): over 4096 walks each is drawn 1024 +- 166 times
    (6 binomial standard deviations, 6 * sqrt(4096 * 0.25 * 0.75))."""
    picks = pair_run["first_pick"]
    assert sum(picks) == 4096 and all(p == 0 for p in picks[4:]), picks
    for k in range(4):
        assert abs(picks[k] - 1024) <= 166, picks
