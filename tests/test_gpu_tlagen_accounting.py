"""What a run on the generated path reports, number for number (MI355X).

The generated path fills no Result.kernels, so tests/test_gpu_kernel_accounting.py cannot pin its
host code.  tests/golden/tlagen_run_accounting.json holds, per case, what the build before
TlagenBackend was given the other backends' shape (a Search struct, named steps, one launch site,
DevOwner for the device resources) reported: verdict, violated invariant, error text, exit code,
depth, generated, distinct, left on queue, every level's (states, generated), n_launches, the
per-action counts and the trace text.  Each case is the repo's smallest model of its kind, in TLC's
single-worker FIFO order (workers=1) and in the -workers N order (workers=0): a plain end, a
violation (workers=0: the event and FIFO re-search path of run()), a VIEW, a deadlock, an evaluation
error of Next, and a prebuilt raft_original source.

Per-action distinct counts are first-come in a workers=0 search that ends without an event (which
producer reaches a state first): their sum is pinned there, and each count everywhere else (a FIFO
search, and a workers=0 search that ended in an event, report TLC's).

The checkpoint case pins the SHA-256 of a checkpoint file (test_checkpoint_bytes_deterministic_in_fifo_order
establishes that the bytes repeat), and with it the code object's key in the file's description.

RAFTMC_RECORD_TLAGEN_ACCOUNTING=<path>: the tests add what this build reports to the JSON file
<path> instead of comparing (record twice, to two paths, and keep the file only if both
recordings are equal).
"""
import hashlib
import json
import os

import pytest

from oracle_util import CONFIGS, GOLDEN
from test_gpu_tlagen import RING, SMALL, gen_source
from tlagen_models import token_ring

pytestmark = pytest.mark.gpu

TLG = os.path.join(CONFIGS, "tlagen")
FIXTURE = os.path.join(GOLDEN, "tlagen_run_accounting.json")
RECORD = os.environ.get("RAFTMC_RECORD_TLAGEN_ACCOUNTING")
COUNTDOWN = os.path.join(TLG, "Countdown.tla")

# name -> (spec, cfg, handle options); every case but the VIEW one runs in both orders
MODELS = {
    "token_ring": (lambda: RING, os.path.join(TLG, "TokenRing.cfg"), {}),
    "token_ring_full": (lambda: RING, os.path.join(TLG, "TokenRing_full.cfg"), {}),
    "token_ring_view": (lambda: gen_source("toy_ring_view"), os.path.join(TLG, "TokenRing_view.cfg"), dict(frontend="generated")),
    "countdown": (lambda: COUNTDOWN, os.path.join(TLG, "Countdown.cfg"), {}),
    "countdown_evalerr": (lambda: COUNTDOWN, os.path.join(TLG, "Countdown_evalerr.cfg"), {}),
    "parity_pair": (lambda: gen_source("parity_pair"), os.path.join(CONFIGS, "parity_pair.cfg"), dict(frontend="generated")),
}
CASES = [(m, w) for m in MODELS for w in ((1,) if m == "token_ring_view" else (1, 0))]
CKPT = "token_ring_w1_checkpoint"


def case_name(model, workers):
    return "%s_w%d" % (model, workers)


def checker(raftmc, model, workers, **kw):
    spec, cfg, opts = MODELS[model]
    return raftmc.ModelChecker(spec(), cfg, workers=workers, **opts, **kw, **SMALL)


def facts(r, workers):
    """what the fixture pins of one run"""
    out = dict(verdict=r.verdict, violated=r.violated, error=r.error, exit_code=r.exit_code, depth=r.depth, generated=r.generated,
               distinct=r.distinct, left_on_queue=r.left_on_queue, levels=[[lv[0], lv[1]] for lv in r.levels],
               n_launches=r.n_launches, act_generated={a: v[0] for a, v in r.actions.items()}, trace_text=r.trace_text)
    if workers == 0 and r.verdict in ("OK", "DEPTH_LIMIT"):   # first-come (the module's docstring)
        out["act_distinct_sum"] = sum(v[1] for v in r.actions.values())
    else:
        out["act_distinct"] = {a: v[1] for a, v in r.actions.items()}
    return out


def pinned(name):
    return json.load(open(RECORD if RECORD else FIXTURE))[name]


def check(name, got):
    print(name, json.dumps(got))
    if not RECORD:
        assert got == pinned(name)
        return
    rec = json.load(open(RECORD)) if os.path.exists(RECORD) else {}
    rec[name] = got
    with open(RECORD, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


def test_fixture_covers_every_case():
    assert sorted(json.load(open(FIXTURE))) == sorted([case_name(m, w) for m, w in CASES] + [CKPT])


@pytest.mark.parametrize("model,workers", CASES)
def test_run_accounting_unchanged(raftmc, model, workers):
    with checker(raftmc, model, workers) as mc:
        got = facts(mc.run(), workers)
    check(case_name(model, workers), got)
    if model == "token_ring":   # the plain end the fixture was chosen for
        want = token_ring()
        assert (got["verdict"], got["distinct"], got["depth"]) == ("OK", want["distinct"], want["depth"]) == ("OK", 4758, 16)
    if model == "token_ring_full":
        assert (got["verdict"], got["violated"], got["depth"]) == ("INVARIANT_VIOLATION", "NotAllFull", 9)


def test_checkpoint_bytes_and_recover(raftmc, tmp_path):
    """The writer's file byte for byte (its description names the code object's key), and a fresh
    handle recovering it reaches the uninterrupted run's result."""
    ck = str(tmp_path / "ring.ckpt")
    with checker(raftmc, "token_ring", 1, max_depth=8) as mc:
        mc.set_checkpoint(ck, 4)
        w = mc.run()
    with checker(raftmc, "token_ring", 1) as mc:
        mc.set_recover(ck)
        r = mc.run()
    got = dict(sha256=hashlib.sha256(open(ck, "rb").read()).hexdigest(), writer=facts(w, 1), recovered=facts(r, 1))
    check(CKPT, got)
    assert (w.verdict, w.depth) == ("DEPTH_LIMIT", 8)
    whole = pinned(case_name("token_ring", 1))
    for key in ("verdict", "generated", "distinct", "depth", "left_on_queue", "act_generated", "act_distinct", "trace_text"):
        assert got["recovered"][key] == whole[key], key
    assert [lv[0] for lv in got["recovered"]["levels"]] == [lv[0] for lv in whole["levels"]]


def dump_lines(mc, path):
    mc.dump_states(path)
    with open(path) as f:
        return f.read().splitlines()


def test_one_handle_many_runs(raftmc, tmp_path):
    """The device buffers a handle keeps between runs.  A handle's order is fixed when it is opened, so
    the two orders alternate on one handle through a -workers N search that ends in an event: run()
    searches in the -workers N order and then again in FIFO order, whose seen-set entries (16 B for 8)
    and per-state bytes (44 for 20) differ, so every buffer is allocated again between the two, and
    again when the next run() starts.  A -workers N search with a plain end runs twice with nothing
    allocated in between.  Either handle gives the fixture's result every time, also after
    release_device_memory()."""
    want = pinned(case_name("token_ring_full", 0))
    with checker(raftmc, "token_ring_full", 0) as mc:
        for step in range(3):
            assert facts(mc.run(), 0) == want, step
            if step == 1:
                mc.release_device_memory()
        assert len(dump_lines(mc, str(tmp_path / "full.txt"))) == want["distinct"]
    want = pinned(case_name("token_ring", 0))
    with checker(raftmc, "token_ring", 0) as mc:
        for step in range(3):
            assert facts(mc.run(), 0) == want, step
            if step == 1:
                mc.release_device_memory()
        assert len(dump_lines(mc, str(tmp_path / "ring.txt"))) == want["distinct"]
