"""Kernel 2g (field_cosetp_k): the second table pair of a block takes the 4 columns it shares with the first from LDS instead of evaluating
them again, and the |p|-only launch has an epilogue of its own.

On a 16-wide array a block runs the pairs sa = 0 and sa = 1 over the same table rows; pair 1's columns ui = 8 .. 11 are pair 0's ui = 0 .. 3 (words
0 .. 3 of every row = pair 0's words 8 .. 11).  The moved words are READ only by a block with KX = 3 positions along x (the fragment of kx = 2, K-step
ka = 0 starts at word 0; with KX <= 2 the lowest word read is 2), and the last table row only with KY = 11: the base shape here -- a 16 x 16 array at
3 mm pitch on a mirror-folded 1 mm grid of 36 x 64 voxels -- has both (asserted on the host with the partition's own arithmetic).

Every case: the whole |p| volume against the fp64 C oracle (TOL_P; the stated e4m3 bound where the variant says fp8corr), |p| alone against the
bits of the two-output launch, and -- in one child process on the debug library -- the bits with and without OLX_EXP_CP_NOREUSE=1 (every pair
filled in full) and an empty bounds report."""
import os
import subprocess
import sys

import numpy as np
import pytest

from openlifu_amd import _native as nat
from oracle import c_oracle as co

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F0, C, RHO, P0 = 400e3, 1500.0, 1000.0, 1e5
TOL_P = 1e-5            # the gate of the lattice tests (tests/test_gpu_field.py)
FP8_BOUND = 7.5e-6      # include/olx.h (olx_field_plan): what a plan that names "fp8corr" promises against the volume maximum
PITCH = 3               # voxels (1 mm grid, 3 mm pitch)
KXW, KYW = 3, 11        # positions of a block along x / y: cos_kxw(2), COS_KYW (olx_params.h)
FOCI3 = [[1e-3, 2e-3, 30e-3], [-3e-3, 1e-3, 26e-3], [2e-3, -4e-3, 22e-3]]      # test_one_output_only_equals_the_two_output_launch: 3 x 4 mirror images = 12 columns
# without a mirror fold a focus is ONE column: kernel 2g (NT = 2) needs 9 .. 16 of them -- the three foci above and six more
FOCI9 = FOCI3 + [[-2e-3, -3e-3, 24e-3], [4e-3, 1e-3, 28e-3], [0.0, 3e-3, 21e-3], [-4e-3, -1e-3, 32e-3], [3e-3, 3e-3, 25e-3], [-1e-3, -4e-3, 29e-3]]

# name: array nax x nay, grid, z of the first plane [m], grid shift [voxels], foci, fp16 opt-out, absorption [Np/m], e4m3 = the variant must say fp8corr (the headline's
# instantiation), a piece of the variant name
CASES = {
    "base_nz32":      dict(arr=(16, 16), n=(36, 64, 32), e4m3=True, expect="mx2,my2,flat,noclamp"),                 # e4m3 corrections where the rule admits them (foci inside, 256 elements)
    "ragged_nz23":    dict(arr=(16, 16), n=(36, 64, 23), expect="mx2,my2,flat,noclamp"),                 # ragged plane block; waves beyond nz fill and move nothing
    "fp16_corr":      dict(arr=(16, 16), n=(36, 64, 32), fp16=True, expect="mx2,my2,flat,noclamp"),
    "clamp":          dict(arr=(16, 16), n=(36, 64, 32), z0=-4e-3, expect="flat,clamp"),                 # grid through the element plane
    "absorption_dir": dict(arr=(16, 16), n=(36, 64, 32), absorb=40.0, expect="uniform absorption"),      # the DIR instantiation
    "no_mirror_fold": dict(arr=(16, 16), n=(36, 64, 32), shift=(3.0, -2.0), foci=FOCI9, e4m3=True, expect="mx1,my1"),
    "nsa1_8x16":      dict(arr=(8, 16), n=(36, 64, 32), expect="mx2,my2"),                               # one pair per block: no reuse
    "nsa3_20x16":     dict(arr=(20, 16), n=(36, 64, 32), e4m3=True, expect="mx2,my2"),                              # padded to 24 x 16: reuse twice
    "nsbp4_16x32":    dict(arr=(16, 32), n=(36, 64, 32), e4m3=True, expect="mx2,my2"),                              # the predecessor of (1, 0) is (0, 2): every pair in full
}


def block_shapes(n, fold):
    """(KX, KY) of every (x coset, y coset) of the launch: coset_partition and build_coset_blocks (olx_plan.cpp) restated.  Positions of a coset
    are two pitches apart along x and one along y; a fold halves the axis."""
    nx, ny = n[0], n[1]
    x_lo, y_lo = (nx // 2 if fold[0] else 0), (ny // 2 if fold[1] else 0)
    px, my = 2 * PITCH, PITCH
    wx, wy = nx - x_lo, ny - y_lo
    nsx = ((wx + px - 1) // px + KXW - 1) // KXW
    nsy = ((wy + my - 1) // my + KYW - 1) // KYW
    out = []
    for rx in range(px):
        for ry in range(my):
            kx_all = (wx - 1 - rx) // px + 1 if rx < wx else 0
            ky_all = (wy - 1 - ry) // my + 1 if ry < wy else 0
            for sx in range(nsx):
                for sy in range(nsy):
                    out.append(((sx + 1) * kx_all // nsx - sx * kx_all // nsx, (sy + 1) * ky_all // nsy - sy * ky_all // nsy))
    return out


def prepare(ctx, name):
    """Elements, steering (kernel 1 on the device: the library then knows the foci) and the grid of a case."""
    cs = CASES[name]
    nax, nay = cs["arr"]
    a, b = np.meshgrid(np.arange(nax), np.arange(nay), indexing="ij")
    pos_m = np.stack([(a.ravel() - (nax - 1) / 2) * 3.0, (b.ravel() - (nay - 1) / 2) * 3.0, np.zeros(nax * nay)], axis=1) * 1e-3
    area = np.full(nax * nay, 2.7 * 2.7 * 1e-6)
    ctx.set_elements(pos_m, np.tile([0.0, 0.0, 1.0], (nax * nay, 1)), area)
    foci = np.asarray(cs.get("foci", FOCI3))
    d, ap = ctx.bf_solve(foci, C)
    n = cs["n"]
    sh = cs.get("shift", (0.0, 0.0))
    xs = ((np.arange(n[0]) - (n[0] - 1) / 2) + sh[0]) * 1e-3
    ys = ((np.arange(n[1]) - (n[1] - 1) / 2) + sh[1]) * 1e-3
    zs = cs.get("z0", 5e-3) + np.arange(n[2]) * 1e-3
    ctx.field_absorption(cs.get("absorb", 0.0))
    return cs, pos_m, area, foci, d, ap, (xs, ys, zs)


def launch(ctx, cs, coords, flags):
    """Plan and launch; returns the variant name and the |p| volumes [focus]."""
    xs, ys, zs = coords
    ctx.field_plan((xs[0], ys[0], zs[0]), (1e-3,) * 3, cs["n"], F0, C, RHO, P0, flags=flags | (nat.FIELD_FP16_CORRECTION if cs.get("fp16") else 0))
    name = ctx.field_variant()
    assert "field_cosetp_k<nt2" in name and cs["expect"] in name, name
    assert ("fp8corr" in name) == bool(cs.get("e4m3")), name      # the e4m3 rule admits the cases marked e4m3 (foci inside the planes, >= 256 equally driven elements) and no other
    ctx.field_launch()
    return name, ctx.field_fetch_all(want=("pmag",))["pmag"]


def test_the_base_shape_reads_the_moved_words_and_the_last_table_row():
    """KX = 3 (the moved words 0 .. 3 are read) and KY = 11 (table row 25 is read) in the folded shape; the unfolded grid is cut into parts of the same size."""
    folded = block_shapes((36, 64, 32), (True, True))
    assert max(kx for kx, _ in folded) == 3 and max(ky for _, ky in folded) == 11 and (3, 11) in folded, folded
    assert all(kx * ky <= 40 for kx, ky in folded)
    plain = block_shapes((36, 64, 32), (False, False))
    assert (3, 11) in plain and all(kx <= 3 and ky <= 11 for kx, ky in plain), plain


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_volume_matches_the_oracle_and_p_alone_has_the_bits_of_both_outputs(ctx, case, monkeypatch):
    """Full-volume |p| parity against the fp64 C oracle with the product's launch (|p| alone since the intensity is derived: the |p|-only
    epilogue), and the same bits from the two-output instantiation (OLX_INTENSITY_STORED=1 at plan time keeps the stored intensity)."""
    cs, pos_m, area, foci, d, ap, coords = prepare(ctx, case)
    monkeypatch.delenv("OLX_INTENSITY_STORED", raising=False)
    name, p_only = launch(ctx, cs, coords, nat.OUT_PMAG)
    monkeypatch.setenv("OLX_INTENSITY_STORED", "1")
    _, both = launch(ctx, cs, coords, nat.OUT_PMAG | nat.OUT_INTENSITY)
    monkeypatch.delenv("OLX_INTENSITY_STORED")
    assert np.array_equal(p_only, both)
    tol = FP8_BOUND if "fp8corr" in name else TOL_P
    xs, ys, zs = coords
    h = 1e-3
    worst = 0.0
    for f in range(len(foci)):
        ref = np.abs(co.field_on_grid(xs, ys, zs, pos_m, area, d[f], ap[f], F0, C, P0, dmin=0.5 * h, absorption=cs.get("absorb", 0.0)))
        err = np.abs(p_only[f].reshape(ref.shape) - ref).max() / ref.max()
        worst = max(worst, err)
    print(f"{case}: {name.strip()[:90]} | worst |p| error {worst:.3e} of the volume maximum (gate {tol:.1e})")
    assert worst <= tol, (case, worst)
    ctx.field_absorption(0.0)


_CHILD = r"""
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
from openlifu_amd import _native as nat
import test_gpu_cosetp_table_reuse as T
assert "libolx_dbg" in os.path.basename(nat.LIB_PATH), nat.LIB_PATH
for case in T.CASES:
    ctx = nat.Context(0)
    cs, pos_m, area, foci, d, ap, coords = T.prepare(ctx, case)
    os.environ.pop("OLX_EXP_CP_NOREUSE", None)
    name, reuse = T.launch(ctx, cs, coords, nat.OUT_PMAG)
    os.environ["OLX_EXP_CP_NOREUSE"] = "1"
    name_full, full = T.launch(ctx, cs, coords, nat.OUT_PMAG)
    os.environ.pop("OLX_EXP_CP_NOREUSE", None)
    assert ",noreuse>" in name_full and "noreuse" not in name, (name, name_full)      # the pin was honoured: the two launches are not the same path
    ctx.sync()          # the debug library reports accesses outside their extent here
    ctx.close()
    if not (np.array_equal(reuse, full) and np.isfinite(reuse).all() and reuse.max() > 0):
        print("DIFFERS:", case, name)
        sys.exit(3)
    print("SAME BITS:", case)
sys.exit(0)
"""


@pytest.mark.gpu
def test_reuse_gives_the_bits_of_the_full_fill_inside_the_extents_in_the_debug_library():
    """lib/libolx_dbg.so honours OLX_EXP_CP_NOREUSE=1 (every pair filled in full) and checks every instrumented index: all cases in ONE child process."""
    lib = os.path.join(ROOT, "openlifu-python_amd", "lib", "libolx_dbg.so")
    env = dict(os.environ, OLX_LIB_PATH=lib)
    for k in ("OLX_FIELD_VARIANT", "OLX_FP8_CORRECTION", "OLX_EXP_KGRP", "OLX_INTENSITY_STORED", "OLX_EXP_CP_NOREUSE"):
        env.pop(k, None)
    code = _CHILD % (ROOT, os.path.join(ROOT, "openlifu-python_amd"), os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, (r.returncode, tail)
    assert tail.count("SAME BITS:") == len(CASES), tail
