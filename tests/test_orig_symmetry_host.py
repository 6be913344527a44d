"""SYMMETRY Permutations(Server) for raft_original on the host (no GPU): the orbit fingerprint
S::fp_sym against S::permute (csrc/orig_spec.h, the header the kernels compile) through
tests/native/orig_sym_host.cpp, the symmetric host BFS against tests/golden/orig_symmetry.json
(written by tests/golden/make_orig_symmetry.py from the generated front end's host BFS, a second
implementation compiled from the unmodified reference text), and the boundary (mc_open)."""
import ctypes
import json
import os
import subprocess

import pytest

from oracle_util import CONFIGS, GOLDEN, ORIG_MC, ROOT, cfg_variant, native_build_dir

SYM_MC = os.path.join(CONFIGS, "raft_original_sym_mc.tla")
FIXTURE = json.load(open(os.path.join(GOLDEN, "orig_symmetry.json")))
# (N, NV, MaxTerm, MaxLogLen, MaxMsgDomain) of each cfg
SHAPES = {"parity_pair": (2, 1, 2, 1, 5), "parity_trio": (3, 2, 3, 2, 2), "c1": (3, 1, 2, 1, 2), "c5v2": (5, 2, 3, 3, 8),
          "c5e_noleader": (5, 2, 2, 4, 6)}
UNSYMMETRIC_DISTINCT = {"parity_pair": 20938, "parity_trio": 42546}   # tests/golden/orig_parity.json
from test_tlagen import needs_ref, needs_tool  # noqa: E402


def build_sym_host(shape):
    """Compile tests/native/orig_sym_host.cpp for one shape (as test_sim_host builds orig_sim_host.cpp)."""
    out = os.path.join(native_build_dir(), "orig_sym_host_%d%d%d%d%d" % shape)
    csrc = os.path.join(ROOT, "raft-tla_amd", "csrc")
    src = [os.path.join(ROOT, "tests", "native", "orig_sym_host.cpp"), os.path.join(csrc, "model.cpp"), os.path.join(csrc, "orig_model.cpp")]
    deps = src + [os.path.join(csrc, h) for h in ("orig_spec.h", "orig_text.h", "sim_rng.h", "common.h", "model.h")]
    if os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps):
        return out
    tmp = "%s.%d" % (out, os.getpid())
    subprocess.run(["g++", "-O2", "-std=c++17", "-DSHAPE_N=%d" % shape[0], "-DSHAPE_NV=%d" % shape[1], "-DSHAPE_MT=%d" % shape[2],
                    "-DSHAPE_ML=%d" % shape[3], "-DSHAPE_MK=%d" % shape[4], "-o", tmp, *src], check=True)
    os.replace(tmp, out)
    return out


def sym_host(name, *args, cfg=None):
    out = subprocess.run([build_sym_host(SHAPES[name]), cfg or os.path.join(CONFIGS, name + ".cfg"), *map(str, args)],
                         capture_output=True, text=True, check=True, timeout=600).stdout
    return json.loads(out.strip().splitlines()[-1])


def sym_cfg(name, **kw):
    """configs/<name>.cfg with the SYMMETRY line added (a temp file; the caller unlinks it)."""
    return cfg_variant(os.path.join(CONFIGS, name + ".cfg"), append="SYMMETRY ServerSymmetry\n", **kw)


def clean(c):
    return (c["disagreements"], c["bad_fp"], c["bad_inverse"], c["bad_pack"]) == (0, 0, 0, 0)


@pytest.mark.parametrize("name", ["parity_pair", "parity_trio"])
def test_fp_sym_is_the_orbit_on_every_reachable_state(name):
    """Every state of the unsymmetric BFS, all N! permutations: fp_sym is constant on the orbit, permute
    is inverted by the inverse permutation, a permuted state is canonical and survives pack/unpack,
    the partition by fp_sym is the partition by the least packed image (0 disagreements), and the
    orbit sizes N!/|stabiliser| sum to the unsymmetric distinct count."""
    c = sym_host(name, "--check")
    assert clean(c), c
    assert c["states"] == UNSYMMETRIC_DISTINCT[name] and c["orbit_sum"] == UNSYMMETRIC_DISTINCT[name], c
    assert c["orbits"] == FIXTURE[name]["distinct"], c


def test_fp_sym_on_five_server_walks_with_elections():
    """The states along 64 seeded walks of 64 states of c5e_noleader.cfg (5 servers, 120 permutations,
    the compact election records), re-walked in the harness: the same properties.  Uniform walks of
    this model from Init hold no election (measured: none in 64 walks of 64 states), so every other
    walk starts behind the scripted shortest first election, and the cfg's NoLeader is taken out so
    that the walks go on with a leader."""
    cfg = cfg_variant(os.path.join(CONFIGS, "c5e_noleader.cfg"), replace=[("    NoLeader\n", "")])
    try:
        c = sym_host("c5e_noleader", "--check-walks", 64, 64, cfg=cfg)
    finally:
        os.unlink(cfg)
    assert clean(c) and c["permutations"] == 120 and c["states"] > 1000 and c["with_elections"] > 500, c


@pytest.mark.parametrize("name", sorted(FIXTURE))
def test_symmetric_host_bfs_matches_fixture(name):
    g = FIXTURE[name]
    r = sym_host(name, *(["--max-depth", g["max_depth"]] if g["max_depth"] else []))
    assert r["err"] == 0 and r["verdict"] == g["verdict"], r
    assert (r["generated"], r["distinct"], r["depth"], r["levels"]) == (g["generated"], g["distinct"], g["depth"], g["levels"])
    assert sum(v[0] for v in r["actions"].values()) == g["generated"] - 1
    assert sum(v[1] for v in r["actions"].values()) == g["distinct"] - 1


@needs_tool
@needs_ref
@pytest.mark.parametrize("name", ["parity_trio", "c1"])
def test_fixture_reproduced_by_generated_path(name):
    from test_tlagen import generate, host_bfs
    g = FIXTURE[name]
    cfg = sym_cfg(name)
    try:
        r = host_bfs(generate(SYM_MC, cfg))
    finally:
        os.unlink(cfg)
    assert r["verdict"] == "OK" and r["err"] == 0
    assert (r["generated"], r["distinct"], r["depth"], r["levels"]) == (g["generated"], g["distinct"], g["depth"], g["levels"])


# ---------------------------------------------------------------- the boundary (mc_open only: no device)
def open_error(raftmc, spec, cfg, **kw):
    try:
        with pytest.raises(raftmc.RaftMCError) as e:
            raftmc.ModelChecker(spec, cfg, **kw)
    finally:
        os.unlink(cfg)
    return e.value


def test_wrapper_with_symmetry_opens(raftmc):
    cfg = sym_cfg("c2")
    try:
        with raftmc.ModelChecker(SYM_MC, cfg) as mc:
            d = mc.describe()
    finally:
        os.unlink(cfg)
    assert d["symmetry"] is True and d["permutations"] == 6 and d["spec"] == "raft_original", d
    with raftmc.ModelChecker(SYM_MC, os.path.join(CONFIGS, "c2.cfg")) as mc:   # the wrapper without the line: no symmetry
        assert "symmetry" not in mc.describe()


def test_symmetry_over_value_is_refused(raftmc, tmp_path):
    tla = tmp_path / "raft_original_valsym_mc.tla"
    tla.write_text(open(SYM_MC).read().replace("MODULE raft_original_sym_mc", "MODULE raft_original_valsym_mc")
                   .replace("EXTENDS raft_original_mc, TLC", "EXTENDS TLC").replace("Permutations(Server)", "Permutations(Value)"))
    e = open_error(raftmc, str(tla), sym_cfg("c2"))
    assert e.code == -4 and "Permutations(Value)" in str(e), str(e)


def test_union_of_permutation_sets_is_refused(raftmc, tmp_path):
    tla = tmp_path / "raft_original_unionsym_mc.tla"
    tla.write_text(open(SYM_MC).read().replace("MODULE raft_original_sym_mc", "MODULE raft_original_unionsym_mc")
                   .replace("EXTENDS raft_original_mc, TLC", "EXTENDS TLC")
                   .replace("Permutations(Server)", "Permutations(Server) \\cup Permutations(Value)"))
    e = open_error(raftmc, str(tla), sym_cfg("c2"))
    assert e.code == -4 and "exactly Permutations(Server)" in str(e), str(e)


def test_undefined_symmetry_name_is_refused(raftmc):
    e = open_error(raftmc, SYM_MC, cfg_variant(os.path.join(CONFIGS, "c2.cfg"), append="SYMMETRY NoSuchSet\n"))
    assert e.code == -4 and "NoSuchSet" in str(e), str(e)
    e = open_error(raftmc, ORIG_MC, sym_cfg("c2"))   # the plain wrapper does not define ServerSymmetry
    assert e.code == -4 and "ServerSymmetry" in str(e), str(e)


def test_view_is_refused(raftmc):
    e = open_error(raftmc, SYM_MC, cfg_variant(os.path.join(CONFIGS, "c2.cfg"), append="VIEW vars\n"))
    assert e.code == -4 and "VIEW" in str(e), str(e)


def test_count_final_level_with_symmetry_is_refused(raftmc):
    e = open_error(raftmc, SYM_MC, sym_cfg("c2"), workers=0, max_depth=5, count_final_level=True)
    assert e.code == -4 and "count_final_level" in str(e), str(e)


def test_two_gpus_with_symmetry_is_refused(raftmc):
    e = open_error(raftmc, SYM_MC, sym_cfg("c2"), workers=0, n_gpus=2, same_device=True)
    assert e.code == -4 and "one GPU" in str(e), str(e)


def test_sharded_entry_points_refuse_symmetry(raftmc):
    """mc_shard_open and the sharded runs refuse before they touch a device."""
    cfg = sym_cfg("c1")
    try:
        with raftmc.ModelChecker(SYM_MC, cfg, workers=0) as mc:
            mc.lib.mc_shard_open.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32]
            assert mc.lib.mc_shard_open(mc.h, 0, 1) == -4 and b"one GPU" in mc.lib.mc_last_error(mc.h)
            mc.lib.mc_shard_run_loopback.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int32]
            arr = (ctypes.c_void_p * 1)(mc.h)
            assert mc.lib.mc_shard_run_loopback(arr, 1) == -4 and b"one GPU" in mc.lib.mc_last_error(mc.h)
    finally:
        os.unlink(cfg)
