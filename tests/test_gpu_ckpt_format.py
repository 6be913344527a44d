"""The checkpoint files of both spec families, byte for byte (MI355X).

TLC's single-worker FIFO order makes a checkpoint deterministic: the same model, seed and depth
write the same bytes on every run.  tests/golden/ckpt_format.json holds the size and SHA-256 of
four such files as the build before the shared state store and checkpoint framing
(csrc/state_store.h, csrc/ckpt_file.h) wrote them; the files written today must be those.
"""
import hashlib
import json
import os

import pytest

from oracle_util import CONFIGS, GOLDEN, ORIG_MC
from test_gpu import FIXTURES, SMALL, _slot_bytes, states_sha
from test_gpu_membership import FIX, SMALL as MEMB_SMALL, open_case

pytestmark = pytest.mark.gpu

WANT = json.load(open(os.path.join(GOLDEN, "ckpt_format.json")))
C1 = os.path.join(CONFIGS, "c1.cfg")
SEED = 0xC0FFEE
DEPTH = 6


def _store_slots(levels):
    """test_spill_state_set_c1's sizing: 1.3 x the largest two consecutive levels"""
    return int(max(x + y for x, y in zip(levels, levels[1:])) * 1.3)


def c1_spill_store(raftmc):
    """a store that spills once before depth 6: sized for the levels the depth-6 search stores (the
    spill rule predicts level 6 from the growth so far with a 1.5x margin, and that does not fit)"""
    slots = _store_slots(FIXTURES["c1"]["levels"][:DEPTH])
    assert slots > sum(FIXTURES["c1"]["levels"][:DEPTH])       # full it is not: only the prediction spills
    return slots * _slot_bytes(raftmc, C1)


def write_c1(raftmc, path, **sizes):
    with raftmc.ModelChecker(ORIG_MC, C1, workers=1, seed=SEED, max_depth=DEPTH, **sizes) as mc:
        mc.set_checkpoint(path, 1)
        r = mc.run()
    assert r.verdict == "DEPTH_LIMIT", r.error


def write_memb(raftmc, case, path):
    """test_membership_checkpoint_recover's first half"""
    with open_case(raftmc, FIX[case], max_depth=9, seed=11, **MEMB_SMALL) as mc:
        mc.set_checkpoint(path, 1)
        r = mc.run()
    assert r.verdict == "DEPTH_LIMIT", r.error


# one per family header and, for tlc_membership, per sym_tlc word of the header
WRITERS = {
    "c1": lambda raftmc, path: write_c1(raftmc, path, **SMALL),
    "c1_spilled": lambda raftmc, path: write_c1(raftmc, path, fp_table_bytes=1 << 26, state_store_bytes=c1_spill_store(raftmc)),
    "memb_two@16": lambda raftmc, path: write_memb(raftmc, "memb_two@16", path),
    "tlc:membership_shipped@16": lambda raftmc, path: write_memb(raftmc, "tlc:membership_shipped@16", path),
}


def file_id(path):
    data = open(path, "rb").read()
    return {"size": len(data), "sha256": hashlib.sha256(data).hexdigest()}


def test_golden_covers_every_configuration():
    assert sorted(WANT) == sorted(WRITERS)


@pytest.mark.parametrize("name", sorted(WRITERS))
def test_checkpoint_bytes_unchanged(raftmc, name, tmp_path):
    ck = str(tmp_path / "f.ckpt")
    WRITERS[name](raftmc, ck)
    got = file_id(ck)
    print(name, got)
    assert got == WANT[name]
    assert not os.path.exists(ck + ".tmp")


def test_spilled_checkpoint_resumes_to_the_oracles_state_set(raftmc, tmp_path):
    """The spilled depth-6 checkpoint, resumed into a store that spills again before the search
    ends (test_spill_state_set_c1's): mc_dump_states reads the host segments and the device part
    in global-id order and gives the oracle's state set."""
    g = FIXTURES["c1"]
    ck = str(tmp_path / "s.ckpt")
    WRITERS["c1_spilled"](raftmc, ck)
    slots = _store_slots(g["levels"])
    assert slots < g["distinct"]
    with raftmc.ModelChecker(ORIG_MC, C1, workers=1, fp_table_bytes=1 << 26, state_store_bytes=slots * _slot_bytes(raftmc, C1)) as mc:
        mc.set_recover(ck)
        r = mc.run()
        sha, n = states_sha(mc)
    assert (r.verdict, r.generated, r.distinct, r.depth) == ("OK", g["generated"], g["distinct"], g["depth"]), r.error
    assert n == g["distinct"] and sha == g["states_sha256"]
