"""TLC -checkpoint / -recover on the generated path (MI355X): a search cut at depth k
by max_depth writes its checkpoint (ckpt_file.h GenHead: the stored states packed in id order), a
fresh handle recovers it -- the states uploaded, the seen-set rebuilt from them by tlg_rebuild_k
(tlagen_kernels.h) -- and goes on to what an uninterrupted run of the same build and the
independent fixtures give.  Every test here is a refusal (MC_E_UNSUPPORTED) on a build without it."""
import json
import os
import subprocess

import pytest

from oracle_util import CONFIGS, GOLDEN, ORIG_MC
from tlagen_models import token_ring

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "raft-tla_amd", "_build", "tlagen_co")
CLI = os.path.join(ROOT, "raft-tla_amd", "_build", "raftmc")
TLG = os.path.join(CONFIGS, "tlagen")
RING = os.path.join(TLG, "TokenRing.tla")
RING_CFG = os.path.join(TLG, "TokenRing.cfg")
SMALL = dict(fp_table_bytes=1 << 26, state_store_bytes=1 << 30)
WAVES1_LANES = 16384   # RAFTMC_TLAGEN_WAVES=1 on the MI355X's 256 CUs: one wave of 64 lanes per CU


def gen_source(name):
    p = os.path.join(GEN, name + ".gen.hip")
    if not os.path.exists(p):
        pytest.skip(p + " not built (raft-tla_amd/csrc/tlagen/prebuild.py)")
    return p


def ring_fixture(view=False):
    w = token_ring(view=view)
    return dict(verdict="OK", generated=w["generated"], distinct=w["distinct"], depth=w["depth"], levels=w["levels"],
                act_generated={a: v[0] for a, v in w["actions"].items()}, act_distinct={a: v[1] for a, v in w["actions"].items()})


def memb_fixture():
    from test_tlagen import memb_actions_as_generated
    g = json.load(open(os.path.join(GOLDEN, "memb_parity.json")))["tlc:memb_two@16"]
    return dict(verdict="DEPTH_LIMIT", generated=g["generated"], distinct=g["distinct"], depth=g["depth"], levels=g["levels"],
                act_distinct={a: v[1] for a, v in memb_actions_as_generated(g["actions"]).items()})


def trio_fixture():
    g = json.load(open(os.path.join(GOLDEN, "orig_parity.json")))["parity_trio"]
    return dict(verdict="OK", generated=g["generated"], distinct=g["distinct"], depth=g["depth"], levels=g["levels"],
                act_generated={"Next": g["generated"] - 1}, act_distinct={"Next": g["distinct"] - 1})


# name -> (spec, cfg, handle options, writer depth k, the recovered run's max_depth, fixture, orders, environment)
CASES = {
    "token_ring": (lambda: RING, RING_CFG, {}, 8, 0, ring_fixture, (1, 0), {}),
    "token_ring_view": (lambda: gen_source("toy_ring_view"), os.path.join(TLG, "TokenRing_view.cfg"), dict(frontend="generated"), 6, 0,
                        lambda: ring_fixture(view=True), (1,), {}),
    # SYMMETRY by TLC's rule and a VIEW: the rebuild must give canon_view's fingerprint of the kept representative
    "memb_two": (lambda: gen_source("memb_two_gen"), os.path.join(CONFIGS, "memb_two.cfg"), dict(frontend="generated", deadlock=False),
                 12, 16, memb_fixture, (1,), {}),
    # one wave per CU, so the rebuild's grid-stride loop makes more than one trip (total > lanes, asserted below)
    "parity_trio": (lambda: gen_source("parity_trio"), os.path.join(CONFIGS, "parity_trio.cfg"), dict(frontend="generated"), None, 0,
                    trio_fixture, (1, 0), {"RAFTMC_TLAGEN_WAVES": "1"}),
}


def trio_cut(levels):
    """parity_trio's writer depth: the issue names 8 of 15 together with `total > lanes`, but 11,858
    states are stored at depth 8 and one wave per CU is 16,384 lanes, so the first depth with more
    stored states than lanes is taken (9: 21,143 states), never less than 8."""
    k = next(d for d in range(8, len(levels)) if sum(levels[:d]) > WAVES1_LANES)
    assert sum(levels[:k]) > WAVES1_LANES and k < len(levels)
    return k


def dump_lines(mc, path):
    mc.dump_states(path)
    with open(path) as f:
        return f.read().splitlines()


def write_ckpt(raftmc, spec, cfg, path, k, workers, every=1, **kw):
    with raftmc.ModelChecker(spec, cfg, workers=workers, max_depth=k, **kw) as mc:
        mc.set_checkpoint(path, every)
        r = mc.run()
    assert r.verdict == "DEPTH_LIMIT", r.error
    assert os.path.exists(path) and not os.path.exists(path + ".tmp")
    return r


def facts(r):
    return dict(verdict=r.verdict, generated=r.generated, distinct=r.distinct, depth=r.depth, levels=[lv[0] for lv in r.levels],
                act_generated={a: v[0] for a, v in r.actions.items()}, act_distinct={a: v[1] for a, v in r.actions.items()})


def fired(got, want):
    """per-action counts as a fixture lists them: an action that never fired (Next itself, where its
    disjuncts are the actions) may be absent there"""
    return {a: v for a, v in got.items() if v or a in want} if isinstance(want, dict) else got


@pytest.mark.parametrize("case,workers", [(c, w) for c in CASES for w in CASES[c][6]])
def test_recover_equals_uninterrupted(raftmc, case, workers, tmp_path, monkeypatch):
    spec, cfg, kw, k, limit, fixture, _, env = CASES[case]
    for name, val in env.items():
        monkeypatch.setenv(name, val)
    spec, want = spec(), fixture()
    if k is None:
        k = trio_cut(want["levels"])
    ck = str(tmp_path / "g.ckpt")
    w = write_ckpt(raftmc, spec, cfg, ck, k, workers, **kw, **SMALL)
    assert [lv[0] for lv in w.levels] == want["levels"][:k]
    with raftmc.ModelChecker(spec, cfg, workers=workers, max_depth=limit, **kw, **SMALL) as mc:
        mc.set_recover(ck)
        r = mc.run()
        got_dump = dump_lines(mc, str(tmp_path / "recovered.txt"))
    with raftmc.ModelChecker(spec, cfg, workers=workers, max_depth=limit, **kw, **SMALL) as mc:
        u = mc.run()
        want_dump = dump_lines(mc, str(tmp_path / "uninterrupted.txt"))
    got, whole = facts(r), facts(u)
    print(case, workers, got)
    assert r.error == "" or r.verdict == "DEPTH_LIMIT", r.error
    keys = ["verdict", "generated", "distinct", "depth", "levels", "act_generated"] + (["act_distinct"] if workers == 1 else [])
    for key in keys:
        assert got[key] == whole[key], key
    for key in keys:   # the independent fixture (per-action counts where it has them; an action that never fired may be absent)
        if key in want:
            assert fired(got[key], want[key]) == want[key], key
    assert len(got_dump) == want["distinct"]
    if workers == 1:   # FIFO ids are deterministic: the same states under the same ids
        assert got_dump == want_dump
    else:
        assert sorted(got_dump) == sorted(want_dump)
    assert r.left_on_queue == u.left_on_queue


def test_checkpoint_bytes_deterministic_in_fifo_order(raftmc, tmp_path):
    """TLC's single-worker FIFO order fixes ids, parents and actions, and the writer packs the words in
    id order: the same model, seed and depth give the same bytes, whatever the checkpoint interval."""
    files = []
    for name, k, every in (("a", 8, 1), ("b", 8, 1), ("c", 9, 1), ("d", 9, 3)):
        p = str(tmp_path / (name + ".ckpt"))
        write_ckpt(raftmc, RING, RING_CFG, p, k, 1, every=every, seed=0xC0FFEE, **SMALL)
        files.append(open(p, "rb").read())
    assert files[0] == files[1]
    assert files[2] == files[3] and files[2] != files[0]
    assert files[0][:8] == b"RAFTMCG1"


EVENT_KEYS = ("verdict", "violated", "depth", "generated", "distinct", "left_on_queue", "exit_code", "trace_text")


@pytest.mark.parametrize("workers", [1, 0])
def test_recover_to_an_event(raftmc, workers, tmp_path):
    """NotAllFull is violated (TokenRing_full.cfg): the recovered search stops where the uninterrupted
    one does, with TLC's counters and counterexample; -workers N searches the event again in FIFO
    order from Init, and leaves its own checkpoint on disk as it wrote it."""
    cfg = os.path.join(TLG, "TokenRing_full.cfg")
    ck = str(tmp_path / "e.ckpt")
    write_ckpt(raftmc, RING, cfg, ck, 4, workers, **SMALL)
    with raftmc.ModelChecker(RING, cfg, workers=workers, **SMALL) as mc:
        mc.set_recover(ck)
        if workers == 0:
            mc.set_checkpoint(ck, 1)
        r = mc.run()
    with raftmc.ModelChecker(RING, cfg, workers=workers, **SMALL) as mc:
        u = mc.run()
    assert u.verdict == "INVARIANT_VIOLATION" and u.violated == "NotAllFull"
    for key in EVENT_KEYS:
        assert getattr(r, key) == getattr(u, key), key
    assert r.actions == u.actions
    if workers == 0:   # the FIFO re-search wrote nothing: the file is still the -workers N search's
        with raftmc.ModelChecker(RING, cfg, workers=1, **SMALL) as mc:
            mc.set_recover(ck)
            with pytest.raises(raftmc.RaftMCError) as e:
                mc.run()
        assert e.value.code == -1 and "-workers N" in str(e.value)


def test_recover_to_a_deadlock(raftmc, tmp_path):
    spec, cfg = os.path.join(TLG, "Countdown.tla"), os.path.join(TLG, "Countdown.cfg")
    ck = str(tmp_path / "d.ckpt")
    write_ckpt(raftmc, spec, cfg, ck, 2, 1, **SMALL)
    with raftmc.ModelChecker(spec, cfg, workers=1, **SMALL) as mc:
        mc.set_recover(ck)
        r = mc.run()
    assert (r.verdict, r.depth, r.exit_code) == ("DEADLOCK", 4, 11)
    assert r.trace_text.count("/\\ x = ") == 4


def overflowed_writer(raftmc, ck, text, **sizes):
    with raftmc.ModelChecker(RING, RING_CFG, workers=0, **sizes) as mc:
        mc.set_checkpoint(ck, 1)
        w = mc.run()
    assert w.verdict == "CAPACITY_OVERFLOW" and w.error == text, (w.verdict, w.error)
    assert os.path.exists(ck) and not os.path.exists(ck + ".tmp")
    return w


def recovered_whole_ring(raftmc, ck, want):
    with raftmc.ModelChecker(RING, RING_CFG, workers=0, **SMALL) as mc:
        mc.set_recover(ck)
        r = mc.run()
    assert r.verdict == "OK", r.error
    assert (r.generated, r.distinct, r.depth, [lv[0] for lv in r.levels]) == (want["generated"], want["distinct"], want["depth"], want["levels"])
    assert fired({a: v[0] for a, v in r.actions.items()}, want["act_generated"]) == want["act_generated"]
    return r


def ckpt_depth(path):
    import struct
    return struct.unpack_from("<q", open(path, "rb").read(120), 8 + 6 * 8 + 8 + 2 * 8)[0]   # GenHead.depth


def test_recover_after_store_overflow(raftmc, tmp_path):
    """What a user does after "state store full": the last checkpoint, written before the overflow, into
    a larger store.  The store is a quarter of the fixture's states (140 B of store per state slot: 20 B
    of bookkeeping and 30 words), so it fills part-way whatever a state's width."""
    want = ring_fixture()
    ck = str(tmp_path / "s.ckpt")
    overflowed_writer(raftmc, ck, "state store full", fp_table_bytes=1 << 26, state_store_bytes=140 * (want["distinct"] // 4))
    assert 3 <= ckpt_depth(ck) < want["depth"]
    recovered_whole_ring(raftmc, ck, want)


def test_recover_after_seen_set_overflow(raftmc, tmp_path):
    want = ring_fixture()
    slots = 1
    while slots * 2 <= want["distinct"] // 2:
        slots *= 2
    assert sum(want["levels"][:3]) < slots < want["distinct"]
    ck = str(tmp_path / "t.ckpt")
    overflowed_writer(raftmc, ck, "seen-set full", fp_table_bytes=slots * 8, state_store_bytes=1 << 30)
    assert 3 <= ckpt_depth(ck) < want["depth"]
    recovered_whole_ring(raftmc, ck, want)


def test_recover_into_too_small_a_table(raftmc, tmp_path):
    """A file with more states than the configured seen-set holds: the rebuild's probes are bounded, the
    call returns, and the verdict is the search's own "seen-set full"."""
    g = trio_fixture()
    assert sum(g["levels"][:8]) > (1 << 16) // 8
    spec, cfg = gen_source("parity_trio"), os.path.join(CONFIGS, "parity_trio.cfg")
    ck = str(tmp_path / "p.ckpt")
    write_ckpt(raftmc, spec, cfg, ck, 8, 0, frontend="generated", **SMALL)
    with raftmc.ModelChecker(spec, cfg, workers=0, frontend="generated", fp_table_bytes=1 << 16, state_store_bytes=1 << 30) as mc:
        mc.set_recover(ck)
        r = mc.run()
    assert (r.verdict, r.error) == ("CAPACITY_OVERFLOW", "seen-set full")


def refused(raftmc, code, spec, cfg, path, **kw):
    with raftmc.ModelChecker(spec, cfg, **kw, **SMALL) as mc:
        mc.set_recover(path)
        with pytest.raises(raftmc.RaftMCError) as e:
            mc.run()
    assert e.value.code == code, str(e.value)


def test_refusals(raftmc, tmp_path):
    ring, c1h, c1g = str(tmp_path / "ring.ckpt"), str(tmp_path / "c1_hand.ckpt"), str(tmp_path / "c1_gen.ckpt")
    c1_cfg, c1_gen = os.path.join(CONFIGS, "c1.cfg"), gen_source("c1")
    write_ckpt(raftmc, RING, RING_CFG, ring, 8, 1, **SMALL)
    write_ckpt(raftmc, ORIG_MC, c1_cfg, c1h, 5, 1, **SMALL)
    write_ckpt(raftmc, c1_gen, c1_cfg, c1g, 5, 1, frontend="generated", **SMALL)
    # another model's file (the same module under another cfg), and the two families' files swapped
    refused(raftmc, -1, RING, os.path.join(TLG, "TokenRing_view.cfg"), ring, workers=1)
    refused(raftmc, -1, c1_gen, c1_cfg, c1h, workers=1, frontend="generated")
    refused(raftmc, -1, ORIG_MC, c1_cfg, c1g, workers=1)
    # cut to half its length; not there at all
    data = open(ring, "rb").read()
    half = str(tmp_path / "half.ckpt")
    with open(half, "wb") as f:
        f.write(data[:len(data) // 2])
    refused(raftmc, -2, RING, RING_CFG, half, workers=1)
    refused(raftmc, -2, RING, RING_CFG, str(tmp_path / "absent.ckpt"), workers=1)
    # a handle without any path runs as before
    want = ring_fixture()
    with raftmc.ModelChecker(RING, RING_CFG, workers=1, **SMALL) as mc:
        r = mc.run()
    got = facts(r)
    assert {k: fired(got[k], want[k]) for k in want} == want


def test_cli_checkpoint_and_recover(tmp_path):
    if not os.path.exists(CLI):
        pytest.skip("raftmc CLI not built")
    ck = str(tmp_path / "cli.ckpt")
    common = ["-workers", "1", "-fptable", str(1 << 26), "-store", str(1 << 30), "-config", RING_CFG]

    def cli(*args):
        return subprocess.run([CLI, *common, *args, RING], capture_output=True, text=True, timeout=300)

    def summary(out):
        return [l for l in out.splitlines() if not l.startswith("Finished in")]

    w = cli("-depth", "8", "-checkpoint", "1", "-checkpoint-file", ck)
    assert os.path.exists(ck), w.stderr
    r, u = cli("-recover", ck), cli()
    assert r.returncode == 0 and u.returncode == 0, r.stderr
    assert summary(r.stdout) == summary(u.stdout)
    want = token_ring()
    assert "%d states generated, %d distinct states found, 0 states left on queue." % (want["generated"], want["distinct"]) in r.stdout
