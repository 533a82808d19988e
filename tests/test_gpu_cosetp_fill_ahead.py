"""Kernel 2g (field_cosetp_k), e4m3 instantiations: a wave evaluates the 7 reuse-form table entries of the block's NEXT pair in front of the K-steps of
the current one (behind the barrier that opens them), keeps the 14 words in registers and writes them to LDS behind the barrier that frees the table (fill-ahead).  Same instructions on the same
inputs as the reuse fill of tests/test_gpu_cosetp_table_reuse.py: the bits must not change.

Every case: (a) the whole |p| volume against the fp64 C oracle (TOL_P; the stated e4m3 bound where the variant says fp8corr) and (b) -- all cases
in ONE child process on the debug library -- the bits with and without OLX_EXP_CP_NOFILLAHEAD=1 (the reuse fill as a phase of its own) and an
empty bounds report.  The shapes are the smallest at which a guard of the fill-ahead can go wrong (1 mm grid, 3 mm pitch):

  base / no fold                                      16 x 16 array, 36 x 64 voxels: KX = 3, KY = 11 -- the moved words and the last table row are read
  ragged_nz23_e4m3, clamp_e4m3                        the same grid with nz = 23 (waves 4 .. 7 of the last plane block lie beyond nz: they hold and store nothing) and through
                                                      the element plane (the e4m3 + clamp instantiation), foci inside the planes; in the debug-library child OLX_FP8_CORRECTION=1
                                                      forces the e4m3 products there, so that the fill-ahead path runs whatever the planner's error rule says of these grids
  nz23 / fp16 / clamp / absorption                    fp16 corrections and DIR: these instantiations keep the fill phase (compile-time) -- controls, equal by construction
  nsa3_20x16                                          three pairs per block: fill-ahead twice
  nsa1_8x16, nsbp4_16x32                              nothing ahead / no reuse form: controls, equal by construction
  few_tiles_12x30                                     every block has 5 positions: waves 5 .. 7 have NO tile and must still evaluate and store their planes
  tiny_8x12                                           every block would have <= 2 positions.  The planner's fill rule (2 rows of 16 in use: 25 % < 60 %,
                                                      olx.hip) keeps kernels 2e / 2g off such a grid, so this case checks the launch the planner does pick;
                                                      few_tiles_12x30 is the smallest folded grid the rule admits (fill 62.5 %) and is where the zero-tile
                                                      guard is exercised (weaker than <= 2 positions: waves 5 .. 7 instead of 2 .. 7).  Both facts are asserted on the
                                                      host below."""
import os
import subprocess
import sys

import numpy as np
import pytest

from openlifu_amd import _native as nat
from oracle import c_oracle as co

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_cosetp_table_reuse as R      # noqa: E402  (helpers only: block_shapes, the foci, the gates)

ROOT = R.ROOT
F0, C, RHO, P0 = R.F0, R.C, R.RHO, R.P0
TOL_P, FP8_BOUND = R.TOL_P, R.FP8_BOUND      # 1e-5 of the volume maximum; 7.5e-6 where the variant says fp8corr
COS_NW, COS_P, KXW, KYW = 8, 2, R.KXW, R.KYW   # waves per block, planes per wave, positions of a block along x / y (olx_params.h)
PIN = "OLX_EXP_CP_NOFILLAHEAD"

# name: array, grid, ... as in test_gpu_cosetp_table_reuse.CASES; k2g = the planner launches kernel 2g (16-column tiles); e4m3 True / False = the variant must
# (not) say fp8corr, None = whatever the planner picks; nsa / nsbp / kxy = what the host test below asserts for the shape
FOCI_IN = [[1e-3, 2e-3, 24e-3], [-3e-3, 1e-3, 20e-3], [2e-3, -4e-3, 16e-3]]      # inside 23 planes from z = 5 mm and inside the planes from z = -4 mm
# force = the debug-library child pins OLX_FP8_CORRECTION=1 for the case (the e4m3 products whatever the error rule says; the product library ignores the pin)
CASES = {
    "base_nz32":       dict(arr=(16, 16), n=(36, 64, 32), e4m3=True, expect="mx2,my2,flat,noclamp", nsa=2, nsbp=2, kxy=(3, 11)),
    "ragged_nz23":     dict(arr=(16, 16), n=(36, 64, 23), e4m3=False, expect="mx2,my2,flat,noclamp", nsa=2, nsbp=2, kxy=(3, 11)),      # waves 4 .. 7 of the last plane block lie beyond nz
    "fp16_corr":       dict(arr=(16, 16), n=(36, 64, 32), e4m3=False, fp16=True, expect="mx2,my2,flat,noclamp", nsa=2, nsbp=2, kxy=(3, 11)),
    "clamp":           dict(arr=(16, 16), n=(36, 64, 32), e4m3=False, z0=-4e-3, expect="flat,clamp", nsa=2, nsbp=2, kxy=(3, 11)),
    "absorption_dir":  dict(arr=(16, 16), n=(36, 64, 32), e4m3=False, absorb=40.0, expect="uniform absorption", nsa=2, nsbp=2, kxy=(3, 11)),
    "no_mirror_fold":  dict(arr=(16, 16), n=(36, 64, 32), e4m3=True, shift=(3.0, -2.0), foci=R.FOCI9, fold=False, expect="mx1,my1", nsa=2, nsbp=2, kxy=(3, 11)),
    "nsa3_20x16":      dict(arr=(20, 16), n=(36, 64, 32), e4m3=True, expect="mx2,my2", nsa=3, nsbp=2, kxy=(3, 11)),
    "nsa1_8x16":       dict(arr=(8, 16), n=(36, 64, 32), e4m3=False, expect="mx2,my2", nsa=1, nsbp=2, kxy=(3, 11)),
    "nsbp4_16x32":     dict(arr=(16, 32), n=(36, 64, 32), e4m3=True, expect="mx2,my2", nsa=2, nsbp=4, kxy=(3, 11)),
    "ragged_nz23_e4m3": dict(arr=(16, 16), n=(36, 64, 23), e4m3=None, force=True, foci=FOCI_IN, expect="mx2,my2,flat,noclamp", nsa=2, nsbp=2, kxy=(3, 11)),
    "clamp_e4m3":      dict(arr=(16, 16), n=(36, 64, 32), e4m3=None, force=True, foci=FOCI_IN, z0=-4e-3, expect="flat,clamp", nsa=2, nsbp=2, kxy=(3, 11)),
    "few_tiles_12x30": dict(arr=(16, 16), n=(12, 30, 32), e4m3=True, expect="mx2,my2", nsa=2, nsbp=2, kxy=(1, 5)),
    "tiny_8x12":       dict(arr=(16, 16), n=(8, 12, 32), e4m3=None, k2g=False, expect="", nsa=2, nsbp=2, kxy=(1, 2)),
}


def coset_fill(n, fold=True):
    """Share of the 16 matrix rows of kernel 2e's tiles that hold a voxel: coset_fill / coset_tiles16 (olx.hip, olx_plan.cpp) restated.  Below 0.6 the
    planner keeps the coset kernels (2e, 2g) off the grid."""
    shapes = R.block_shapes(n, (fold, fold))
    wx, wy = (n[0] - n[0] // 2, n[1] - n[1] // 2) if fold else (n[0], n[1])
    return COS_P * wx * wy / (16.0 * sum((COS_P * kx * ky + 15) // 16 for kx, ky in shapes))


def coords_of(cs):
    n = cs["n"]
    sh = cs.get("shift", (0.0, 0.0))
    xs = ((np.arange(n[0]) - (n[0] - 1) / 2) + sh[0]) * 1e-3
    ys = ((np.arange(n[1]) - (n[1] - 1) / 2) + sh[1]) * 1e-3
    zs = cs.get("z0", 5e-3) + np.arange(n[2]) * 1e-3
    return xs, ys, zs


def elements_of(cs):
    nax, nay = cs["arr"]
    a, b = np.meshgrid(np.arange(nax), np.arange(nay), indexing="ij")
    pos_m = np.stack([(a.ravel() - (nax - 1) / 2) * 3.0, (b.ravel() - (nay - 1) / 2) * 3.0, np.zeros(nax * nay)], axis=1) * 1e-3
    return pos_m, np.full(nax * nay, 2.7 * 2.7 * 1e-6)


def prepare(ctx, name):
    """Elements, steering (kernel 1 on the device: the library then knows the foci) and the grid of a case."""
    cs = CASES[name]
    pos_m, area = elements_of(cs)
    ctx.set_elements(pos_m, np.tile([0.0, 0.0, 1.0], (len(pos_m), 1)), area)
    foci = np.asarray(cs.get("foci", R.FOCI3))
    d, ap = ctx.bf_solve(foci, C)
    ctx.field_absorption(cs.get("absorb", 0.0))
    return cs, pos_m, area, foci, d, ap, coords_of(cs)


def launch(ctx, cs, coords):
    """Plan and launch the product's outputs (|p| alone); returns the variant name and the |p| volumes [focus]."""
    xs, ys, zs = coords
    ctx.field_plan((xs[0], ys[0], zs[0]), (1e-3,) * 3, cs["n"], F0, C, RHO, P0, flags=nat.OUT_PMAG | (nat.FIELD_FP16_CORRECTION if cs.get("fp16") else 0))
    name = ctx.field_variant()
    if cs.get("k2g", True):
        assert "field_cosetp_k<nt2" in name and cs["expect"] in name, name
    else:
        assert "field_cosetp_k" not in name, name      # (the fill rule: see the module docstring)
    if cs["e4m3"] is not None:
        assert ("fp8corr" in name) == cs["e4m3"], name
    ctx.field_launch()
    return name, ctx.field_fetch_all(want=("pmag",))["pmag"]


# ---- host tests (no GPU) ----
def test_the_shapes_have_the_blocks_tiles_and_pairs_claimed_for_them():
    """coset_partition / build_coset_blocks restated (block_shapes): (KX, KY) of the largest block, the tiles of every wave, the pairs of a block."""
    for name, cs in CASES.items():
        fold = cs.get("fold", True)
        shapes = R.block_shapes(cs["n"], (fold, fold))
        kx, ky = cs["kxy"]
        assert max(s[0] for s in shapes) == kx and max(s[1] for s in shapes) == ky and (kx, ky) in shapes, (name, shapes)
        assert all(a <= KXW and b <= KYW and a * b <= 40 for a, b in shapes), (name, shapes)
        tiles = [[max(0, (a * b - w + COS_NW - 1) // COS_NW) for w in range(COS_NW)] for a, b in shapes if a * b > 0]
        assert all(max(t) <= 5 for t in tiles), (name, tiles)
        nax, nay = cs["arr"]
        assert ((nax + 7) // 8, ((nay + 7) // 8 + 1) & ~1) == (cs["nsa"], cs["nsbp"]), name      # pairs per block = nsa * nsbp / 2; the reuse form needs nsbp == 2
    # KX = 3: the moved words 0 .. 3 are read; KY = 11: table row 25 is read (tests/test_gpu_cosetp_table_reuse.py)
    assert CASES["base_nz32"]["kxy"] == (3, 11)
    # waves without a tile: every block of few_tiles_12x30 has 5 positions -- waves 5 .. 7 fill their planes and run no tile
    few = [a * b for a, b in R.block_shapes(CASES["few_tiles_12x30"]["n"], (True, True)) if a * b > 0]
    assert few and all(p == 5 for p in few), few
    assert coset_fill(CASES["few_tiles_12x30"]["n"]) >= 0.6
    # ... and on the 8 x 12 grid every block has <= 2 positions (waves 2 .. 7 without a tile), which the planner's fill rule does not hand to kernel 2g
    tiny = [a * b for a, b in R.block_shapes(CASES["tiny_8x12"]["n"], (True, True))]
    assert max(tiny) == 2 and all(p <= 2 for p in tiny), tiny
    assert coset_fill(CASES["tiny_8x12"]["n"]) < 0.6
    assert coset_fill(CASES["base_nz32"]["n"]) >= 0.6 and coset_fill(CASES["no_mirror_fold"]["n"], fold=False) >= 0.6
    # ragged_nz23: the second plane block holds planes 16 .. 22 -- waves 4 .. 7 (planes 24 ..) lie beyond nz
    assert 16 + 4 * COS_P > CASES["ragged_nz23"]["n"][2] > 16 + 3 * COS_P and CASES["ragged_nz23_e4m3"]["n"] == CASES["ragged_nz23"]["n"]


def test_the_variant_name_can_say_nofillahead_only_in_developer_builds():
    """Only this: the product library does not contain the tag `nofillahead` at all (it can never name it), the debug library contains the tag and the
    pin's name.  Whether the pin is honoured -- the name carries the tag exactly when the pin is set, and the launch takes the other path -- is asserted
    on the GPU, in the child process below."""
    lib = os.path.join(ROOT, "openlifu-python_amd", "lib")
    with open(os.path.join(lib, "libolx.so"), "rb") as f:
        product = f.read()
    assert b"nofillahead" not in product      # (the pin's NAME is known to every build: it is part of the key that decides whether a plan is still valid)
    dbg = os.path.join(lib, "libolx_dbg.so")
    if not os.path.exists(dbg):
        pytest.skip("only the product library is built")
    with open(dbg, "rb") as f:
        debug = f.read()
    assert PIN.encode() in debug and b",nofillahead" in debug and b"OLX_EXP_CP_NOREUSE" in debug


def test_the_references_alone_meet_the_preconditions_of_the_gates():
    """Foci inside the planes (and >= 256 equally driven elements) where e4m3 is expected -- what the e4m3 rule and its 7.5e-6 bound presuppose --
    and a finite reference with a positive maximum (the gates are relative to it), computed here for the smallest volume."""
    for name, cs in CASES.items():
        xs, ys, zs = coords_of(cs)
        foci = np.asarray(cs.get("foci", R.FOCI3))
        inside = ((foci[:, 0] >= xs[0]) & (foci[:, 0] <= xs[-1]) & (foci[:, 1] >= ys[0]) & (foci[:, 1] <= ys[-1]) & (foci[:, 2] >= zs[0]) & (foci[:, 2] <= zs[-1])).all()
        if cs["e4m3"] or cs.get("force"):
            assert inside and cs["arr"][0] * cs["arr"][1] >= 256, name
        if name == "ragged_nz23":
            assert not inside      # the focus at z = 30 mm lies above the last plane: fp16 corrections
    cs = CASES["tiny_8x12"]
    pos_m, area = elements_of(cs)
    xs, ys, zs = coords_of(cs)
    f = np.asarray(R.FOCI3[0])
    d = np.linalg.norm(pos_m - f, axis=1)
    ref = np.abs(co.field_on_grid(xs, ys, zs, pos_m, area, (d.max() - d) / C, np.ones(len(pos_m)), F0, C, P0, dmin=0.5e-3, absorption=0.0))
    assert np.isfinite(ref).all() and ref.max() > 0


# ---- GPU ----
@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_volume_matches_the_oracle(ctx, case):
    """Full-volume |p| parity against the fp64 C oracle with the product's launch (fill-ahead wherever the block takes the reuse form)."""
    cs, pos_m, area, foci, d, ap, coords = prepare(ctx, case)
    name, p = launch(ctx, cs, coords)
    assert "nofillahead" not in name, name
    tol = FP8_BOUND if "fp8corr" in name else TOL_P
    xs, ys, zs = coords
    worst = 0.0
    for f in range(len(foci)):
        ref = np.abs(co.field_on_grid(xs, ys, zs, pos_m, area, d[f], ap[f], F0, C, P0, dmin=0.5e-3, absorption=cs.get("absorb", 0.0)))
        worst = max(worst, np.abs(p[f].reshape(ref.shape) - ref).max() / ref.max())
    print(f"{case}: {name.strip()[:90]} | worst |p| error {worst:.3e} of the volume maximum (gate {tol:.1e})")
    assert worst <= tol, (case, worst)
    ctx.field_absorption(0.0)


_CHILD = r"""
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
from openlifu_amd import _native as nat
import test_gpu_cosetp_fill_ahead as T
assert "libolx_dbg" in os.path.basename(nat.LIB_PATH), nat.LIB_PATH
for case in T.CASES:
    ctx = nat.Context(0)
    cs, pos_m, area, foci, d, ap, coords = T.prepare(ctx, case)
    os.environ.pop(T.PIN, None)
    os.environ.pop("OLX_FP8_CORRECTION", None)
    if cs.get("force"):
        os.environ["OLX_FP8_CORRECTION"] = "1"
    name, ahead = T.launch(ctx, cs, coords)
    os.environ[T.PIN] = "1"
    name_pin, own = T.launch(ctx, cs, coords)
    os.environ.pop(T.PIN, None)
    os.environ.pop("OLX_FP8_CORRECTION", None)
    if cs.get("force") or cs["e4m3"]:      # the instantiations that fill ahead
        assert "fp8corr" in name and "fp8corr" in name_pin, (name, name_pin)
    if cs.get("k2g", True):      # the pin was honoured: the two launches are not the same path
        assert ",nofillahead>" in name_pin and "nofillahead" not in name, (name, name_pin)
    ctx.sync()          # the debug library reports accesses outside their extent here
    ctx.close()
    if not (np.array_equal(ahead, own) and np.isfinite(ahead).all() and ahead.max() > 0):
        print("DIFFERS:", case, name)
        sys.exit(3)
    print("SAME BITS:", case, "|", name.strip()[:70])
sys.exit(0)
"""


@pytest.mark.gpu
def test_fill_ahead_gives_the_bits_of_the_fill_phase_inside_the_extents_in_the_debug_library():
    """lib/libolx_dbg.so honours OLX_EXP_CP_NOFILLAHEAD=1 (today's reuse fill between the two barriers) and checks every instrumented index: all cases in ONE child process."""
    lib = os.path.join(ROOT, "openlifu-python_amd", "lib", "libolx_dbg.so")
    env = dict(os.environ, OLX_LIB_PATH=lib)
    for k in ("OLX_FIELD_VARIANT", "OLX_FP8_CORRECTION", "OLX_EXP_KGRP", "OLX_INTENSITY_STORED", "OLX_EXP_CP_NOREUSE", PIN):
        env.pop(k, None)
    code = _CHILD % (ROOT, os.path.join(ROOT, "openlifu-python_amd"), os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, (r.returncode, tail)
    assert tail.count("SAME BITS:") == len(CASES), tail
