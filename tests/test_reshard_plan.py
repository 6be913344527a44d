"""The index arithmetic of recovering a checkpoint at another GPU count (csrc/reshard_plan.h, what
the kernels of csrc/orig_reshard.hip place states with) without a GPU: tests/native/
reshard_plan_check.cpp runs it over a random source, and this file restates the plan by brute force:
states are objects, the canonical order of a level is a sort by (source rank, index in that rank's
store), a state's index among its new owner's is a count over the states before it, and its new parent
is whatever new id its parent object got."""
import os
import random
import subprocess

import pytest

from oracle_util import ROOT, native_build_dir

NONE = (1 << 64) - 1


def build_check():
    out = os.path.join(native_build_dir(), "reshard_plan_check")
    csrc = os.path.join(ROOT, "raft-tla_amd", "csrc")
    src = os.path.join(ROOT, "tests", "native", "reshard_plan_check.cpp")
    deps = [src, os.path.join(csrc, "reshard_plan.h"), os.path.join(csrc, "common.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in deps):
        tmp = "%s.%d" % (out, os.getpid())
        subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", csrc, "-o", tmp, src], check=True)
        os.replace(tmp, out)
    return out


class State:
    def __init__(self, level, src, owner, parent, low):
        self.level, self.src, self.owner, self.parent, self.low = level, src, owner, parent, low
        self.local = self.old_meta = self.new_id = None


def make_source(rng, W, WP, sizes, starved):
    """A search of len(sizes) levels whose states lie on W source ranks as the sharded loop stores
    them: every rank's levels one behind the other.  No state goes to the owner `starved`."""
    owners = [o for o in range(WP) if o != starved] or [0]
    levels, stored = [], [0] * W
    for l, n in enumerate(sizes):
        lv = [State(l, rng.randrange(W), rng.choice(owners), rng.choice(levels[-1]) if l else None, rng.randrange(1 << 24))
              for _ in range(n)]
        for r in range(W):
            mine = [s for s in lv if s.src == r]
            for k, s in enumerate(mine):
                s.local = stored[r] + k
            stored[r] += len(mine)
        levels.append(lv)
    for lv in levels:
        for s in lv:
            s.old_meta = NONE if s.parent is None else (((s.parent.src << 37) | s.parent.local) << 24) | s.low
    return levels


def canonical(lv):
    return sorted(lv, key=lambda s: (s.src, s.local))


def run_plan(tmp_path, W, WP, levels, metas=None):
    text = ["%d %d %d" % (W, WP, len(levels))]
    for l, lv in enumerate(levels):
        text.append(" ".join(str(sum(1 for s in lv if s.src == r)) for r in range(W)))
        for i, s in enumerate(canonical(lv)):
            text.append("%d %d" % (s.owner, s.old_meta if metas is None else metas.get((l, i), s.old_meta)))
    inp = tmp_path / "plan.in"
    inp.write_text("\n".join(text) + "\n")
    r = subprocess.run([build_check(), str(inp)], capture_output=True, text=True)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
    lines = iter(r.stdout.split("\n"))
    got = []
    for lv in levels:
        head = next(lines).split()
        assert head[0] == "level"
        got.append(([int(x) for x in head[1:]], [next(lines).split() for _ in lv]))
    return got


SIZES = [1, 5, 257, 300, 64, 1, 7]   # a level of 1 state, one of 257 (a workgroup and one state), a last level of 7


@pytest.mark.parametrize("W", [1, 2, 3, 8])
@pytest.mark.parametrize("WP", [1, 2, 3, 8])
def test_plan_equals_brute_force(tmp_path, W, WP):
    rng = random.Random(1000 * W + WP)
    starved = WP - 1 if WP > 1 else None           # an owner that receives nothing
    levels = make_source(rng, W, WP, SIZES, starved)
    got = run_plan(tmp_path, W, WP, levels)
    # brute force: new ids
    received = [0] * WP
    for lv in levels:
        begin = list(received)
        for s in canonical(lv):
            before = sum(1 for t in canonical(lv) if t.owner == s.owner and (t.src, t.local) < (s.src, s.local))
            s.new_id = (s.owner << 37) | (begin[s.owner] + before)
        for s in lv:
            received[s.owner] += 1
    seen = set()
    for (counts, rows), lv in zip(got, levels):
        assert counts == [sum(1 for s in lv if s.owner == o) for o in range(WP)] and sum(counts) == len(lv)
        if starved is not None:
            assert counts[starved] == 0
        for (new_id, new_meta), s in zip(rows, canonical(lv)):
            assert int(new_id) == s.new_id
            assert s.new_id not in seen
            seen.add(s.new_id)
            if s.parent is None:
                assert int(new_meta) == NONE
            else:
                m = int(new_meta)
                assert m & ((1 << 24) - 1) == s.low                      # the action byte and the low bits stay
                assert m >> 24 == s.parent.new_id                        # the parent object's new id ...
                assert s.parent.level == s.level - 1                     # ... which lies in the level before
    # every owner's ids are 0 .. its count - 1, and its levels lie one behind the other
    for o in range(WP):
        mine = [s for lv in levels for s in canonical(lv) if s.owner == o]
        assert [s.new_id & ((1 << 37) - 1) for s in mine] == list(range(len(mine)))


@pytest.mark.parametrize("W", [1, 3])
def test_plan_refuses_parents_outside_the_level_before(tmp_path, W):
    """A parent pointer that names a rank the source does not have, an index outside that rank's
    slice of the level before, a state of the same level or of the level before the last one, or any
    parent at all for an initial state, is reported, not indexed with."""
    rng = random.Random(7 + W)
    levels = make_source(rng, W, 2, [2, 40, 90, 30], None)
    lv1, lv2 = canonical(levels[1]), canonical(levels[2])
    tagged = lambda rank, local: ((rank << 37) | local) << 24
    bad = {
        (2, 0): tagged(W, 0),                                   # a rank behind the last
        (2, 1): tagged(7 if W < 8 else 0, 1 << 36),             # far outside
        (2, 2): tagged(lv2[5].src, lv2[5].local),               # a state of its own level
        (2, 3): tagged(canonical(levels[0])[0].src, canonical(levels[0])[0].local),   # the level before the last one
        (2, 4): tagged(lv1[0].src, (1 << 37) - 1),              # the largest index
        (0, 0): tagged(0, 0),                                   # an initial state has no parent
    }
    got = run_plan(tmp_path, W, 2, levels, metas=bad)
    for l, (_, rows) in enumerate(got):
        for i, (_, new_meta) in enumerate(rows):
            assert (new_meta == "bad") == ((l, i) in bad), (l, i, new_meta)
