"""Kernel 2g (field_cosetp_k): the fragment addresses of a wave's <= 5 tiles are formed once per block (byte addresses held in registers across the
pairs; every ds_read_b64 of a tile-step takes its K-step and array offset as an immediate -- in every instantiation), and the wave-uniform tile
guards `t >= ntile` are scalar compares.  Arithmetic, LDS layout and the order of the matrix instructions are the parent's: the bits must not change.

The cases are the smallest grids at which a tile address or a guard can go wrong (1 mm grid, 3 mm pitch: the lattice pitch is 3 voxels); table,
helpers and gates are those of tests/test_gpu_cosetp_fill_ahead.py and tests/test_gpu_cosetp_table_reuse.py:

  base_nz32 (36 x 64 x 32)   (KX, KY) = (3, 11), 33 positions: wave 0 alone owns a fifth tile, kx = 2 reaches the lowest table column, ky = 10 the last row
  few_tiles_12x30            5 positions: waves 5 .. 7 have no tile -- their clamped position must form an in-range address and read nothing
  ragged_nz23_e4m3           waves whose planes lie beyond nz
  clamp_e4m3                 the e4m3 + clamp instantiation (118 registers: it holds the five addresses too, no fall-back form exists)
  fp16_corr, absorption_dir  the fp16-correction and DIR instantiations (the other K-step body: one K-step per group, four 8-byte reads per tile-step)
  no_mirror_fold             MX = MY = 1
  nsa3_20x16, nsbp4_16x32    three pairs; pairs that do not reuse

Every case: (1) the full |p| volume of every focus against the fp64 C oracle at those files' gates -- the product's launch, and for ragged_nz23_e4m3
and clamp_e4m3, where the product's planner may keep the fp16 corrections, ALSO the debug library's launch with the e4m3 products forced (its variant
must say fp8corr), at the gate of a variant that says fp8corr --, (2) an empty bounds report from the debug
library, whose fragment check sees the word index the held byte address stands for, (3) in the debug library the bits with and without
OLX_EXP_CP_NOFILLAHEAD=1 (the same addresses through the other fill path), and the debug library's bits against the product library's wherever
both take the same products.  On the host: the address arithmetic restated, every fragment word index of these shapes inside the table."""
import os
import subprocess
import sys

import numpy as np
import pytest

from openlifu_amd import _native as nat
from oracle import c_oracle as co

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_cosetp_fill_ahead as F       # noqa: E402  (case table, prepare / launch, the pin)
import test_gpu_cosetp_table_reuse as R      # noqa: E402  (block_shapes, the gates)

ROOT = R.ROOT
NAMES = ["base_nz32", "few_tiles_12x30", "ragged_nz23_e4m3", "clamp_e4m3", "fp16_corr", "absorption_dir", "no_mirror_fold", "nsa3_20x16", "nsbp4_16x32"]

# ---- the kernel's address arithmetic restated (k_coset2.hip, olx_params.h) ----
COS_NW, COS_ZB, MT = 8, 16, 5                 # waves per block, planes per block, tiles per wave
TW, ROW0, PSZ, UW = 14, 15, 364, 12           # words per table row, row of offset 0, words per plane table, table columns
T_WORDS = COS_ZB * PSZ
B_BYTES = 2 * 4 * 2 * 128 * 16                # steering stage in front of the two table arrays


def toff_of(wave, t, npos, KY):
    """Word offset of tile t of a wave (wave-uniform); a wave without a tile t forms the address of the block's last position."""
    pos = min(wave + COS_NW * t, npos - 1)
    kx = (pos * (65536 // KY + 1)) >> 16
    return pos, kx, (pos - kx * KY + ROW0) * TW + (UW - 8 - 2 * kx)


def lane_off_of(lane):
    """Per-lane part: plane lane % 16, k-group lane / 16 one table row lower each."""
    return (lane & 15) * PSZ - (lane >> 4) * TW


def kso_of(sl, kb, ka):
    """K-step part: 4 columns per ka, 4 rows per kb, 8 rows per super-block of the pair."""
    return 4 * ka - (4 * kb + 8 * sl) * TW


def test_the_restated_address_arithmetic_alone():
    """The reference first: the magic division is exact for every position a block can have, the documented corners land where the kernel's comments
    say (kx = 2, ka = 0 starts at word 0 of its row; ky = 10 reads up to table row 25), lanes of one ds_read_b64 group meet 32 distinct 8-byte slots."""
    for KY in range(1, R.KYW + 1):
        for pos in range(41):
            assert (pos * (65536 // KY + 1)) >> 16 == pos // KY, (KY, pos)
    assert T_WORDS == 5824 and B_BYTES == 32768 and PSZ == 26 * TW
    # position (kx, ky) = (2, 0) of a (3, 11) block, lane 0, K-step (sl, kb, ka) = (0, 0, 0): row 15, word 0
    pos, kx, toff = toff_of(6, 2, 33, 11)
    assert (pos, kx) == (22, 2) and toff == ROW0 * TW + 0
    # ky = 10 with k-group 0 at (0, 0, .): row 25 = the last table row; k-group 3 of ky = 0 in the pair's second super-block, kb = 1: row 0
    assert (toff_of(2, 1, 33, 11)[2] + lane_off_of(0)) // TW == 25
    assert (toff_of(0, 0, 33, 11)[2] + lane_off_of(48) + kso_of(1, 1, 0)) // TW == 0
    # wave 0 alone owns a fifth tile of 33 positions; a wave beyond the positions is clamped to the last one
    assert [max(0, (33 - w + COS_NW - 1) // COS_NW) for w in range(COS_NW)] == [5, 4, 4, 4, 4, 4, 4, 4]
    assert toff_of(7, 4, 5, 5)[0] == 4
    # 16 planes x 2 k-groups of a ds_read_b64 lane group: 32 distinct 8-byte slots of the 64 LDS banks
    slots = {((lane_off_of(lane) + 168) // 2) % 32 for lane in range(32)}
    assert len(slots) == 32


def test_every_fragment_word_index_of_these_shapes_lies_inside_the_table():
    """All tiles (those a wave does not run included: their address is formed), (sl, kb, ka) groups and lanes of every block shape of the cases: the
    four words a lane reads from either array start in [0, T_WORDS - 4]; as a byte address plus immediate they fit the 16-bit offset field of a DS
    instruction.  (Both pairs of a block read the same indices: the pair changes what the table holds, not where.)"""
    lanes = np.arange(64)
    lane_off = (lanes & 15) * PSZ - (lanes >> 4) * TW
    ksos = np.array([kso_of(sl, kb, ka) for sl in range(2) for kb in range(2) for ka in range(2)])
    seen_lo, seen_hi = T_WORDS, -1
    for name in NAMES:
        cs = F.CASES[name]
        fold = cs.get("fold", True)
        shapes = {s for s in R.block_shapes(cs["n"], (fold, fold)) if s[0] * s[1] > 0}
        assert cs["kxy"] in shapes, (name, shapes)
        for KX, KY in shapes:
            npos = KX * KY
            assert npos <= 40 and KX <= R.KXW and KY <= R.KYW
            for wave in range(COS_NW):
                for t in range(MT):
                    _, kx, toff = toff_of(wave, t, npos, KY)
                    assert 0 <= kx < KX
                    idx = (lane_off[:, None] + toff + ksos[None, :])
                    lo, hi = int(idx.min()), int(idx.max())
                    assert 0 <= lo and hi <= T_WORDS - 4, (name, KX, KY, wave, t, lo, hi)
                    seen_lo, seen_hi = min(seen_lo, lo), max(seen_hi, hi)
                    base = (lane_off + toff) << 2                    # the held byte address
                    assert base.min() >= 0
    imm = B_BYTES + 4 * ksos
    assert imm.min() >= 0 and imm.max() + 4 * T_WORDS + 8 <= 0xFFFF      # hi array, lo array, second 8-byte half
    # the base shape does reach both ends of the table (otherwise this test checks less than it says)
    assert seen_lo == 0 and seen_hi // TW == 25 + 15 * 26, (seen_lo, seen_hi)


# ---- GPU ----
_PRODUCT = {}


def product_launch(case):
    """The product library's launch of a case, once per session: (variant name, |p| [focus], inputs of the oracle)."""
    if case not in _PRODUCT:
        ctx = nat.Context(0)
        try:
            cs, pos_m, area, foci, d, ap, coords = F.prepare(ctx, case)
            name, p = F.launch(ctx, cs, coords)
            ctx.field_absorption(0.0)
        finally:
            ctx.close()
        _PRODUCT[case] = (name, p, (cs, pos_m, area, foci, d, ap, coords))
    return _PRODUCT[case]


def worst_error(p, cs, pos_m, area, d, ap, coords):
    """Largest |p| error over the full volumes of all foci against the fp64 C oracle, as a share of each volume's maximum."""
    xs, ys, zs = coords
    worst = 0.0
    for f in range(len(d)):
        ref = np.abs(co.field_on_grid(xs, ys, zs, pos_m, area, d[f], ap[f], F.F0, F.C, F.P0, dmin=0.5e-3, absorption=cs.get("absorb", 0.0)))
        assert np.isfinite(p[f]).all()
        worst = max(worst, np.abs(p[f].reshape(ref.shape) - ref).max() / ref.max())
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("case", NAMES)
def test_volume_matches_the_oracle(case):
    """(1) Full-volume |p| of every focus against the fp64 C oracle with the product's launch."""
    name, p, (cs, pos_m, area, foci, d, ap, coords) = product_launch(case)
    assert "field_cosetp_k<nt2" in name, name
    tol = R.FP8_BOUND if "fp8corr" in name else R.TOL_P
    worst = worst_error(p, cs, pos_m, area, d, ap, coords)
    print(f"{case}: {name.strip()[:90]} | worst |p| error {worst:.3e} of the volume maximum (gate {tol:.1e})")
    assert worst <= tol, (case, worst)


_CHILD = r"""
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
from openlifu_amd import _native as nat
import test_gpu_cosetp_tile_addr as T
F = T.F
out = %r
assert "libolx_dbg" in os.path.basename(nat.LIB_PATH), nat.LIB_PATH
for case in T.NAMES:
    ctx = nat.Context(0)
    cs, pos_m, area, foci, d, ap, coords = F.prepare(ctx, case)
    for k in (F.PIN, "OLX_FP8_CORRECTION"):
        os.environ.pop(k, None)
    if cs.get("force"):
        os.environ["OLX_FP8_CORRECTION"] = "1"
    name, ahead = F.launch(ctx, cs, coords)
    os.environ[F.PIN] = "1"
    name_pin, own = F.launch(ctx, cs, coords)
    for k in (F.PIN, "OLX_FP8_CORRECTION"):
        os.environ.pop(k, None)
    if cs.get("force") or cs["e4m3"]:      # the e4m3 K-step body
        assert "fp8corr" in name and "fp8corr" in name_pin, (name, name_pin)
    assert ",nofillahead>" in name_pin and "nofillahead" not in name, (name, name_pin)      # the pin was honoured
    ctx.sync()          # the debug library reports accesses outside their extent here
    ctx.close()
    if not (np.array_equal(ahead, own) and np.isfinite(ahead).all() and ahead.max() > 0):
        print("DIFFERS:", case, name)
        sys.exit(3)
    np.save(os.path.join(out, case + ".npy"), ahead)
    np.savez(os.path.join(out, case + "_steer.npz"), d=d, ap=ap)
    with open(os.path.join(out, case + ".txt"), "w") as fh:
        fh.write(name)
    print("SAME BITS:", case, "|", name.strip()[:70])
sys.exit(0)
"""


_DEBUG = {}


def debug_launches(tmp_path_factory):
    """All cases in ONE child process on lib/libolx_dbg.so, once per session: (return code, end of the output, directory of the volumes it saved)."""
    if not _DEBUG:
        out = str(tmp_path_factory.mktemp("tile_addr_dbg"))
        lib = os.path.join(ROOT, "openlifu-python_amd", "lib", "libolx_dbg.so")
        env = dict(os.environ, OLX_LIB_PATH=lib)
        for k in ("OLX_FIELD_VARIANT", "OLX_FP8_CORRECTION", "OLX_EXP_KGRP", "OLX_INTENSITY_STORED", "OLX_EXP_CP_NOREUSE", F.PIN):
            env.pop(k, None)
        code = _CHILD % (ROOT, os.path.join(ROOT, "openlifu-python_amd"), os.path.join(ROOT, "tests"), out)
        r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
        _DEBUG["run"] = (r.returncode, (r.stdout + r.stderr)[-3000:], out)
    return _DEBUG["run"]


@pytest.mark.gpu
def test_debug_library_reports_nothing_and_has_the_bits_of_the_other_fill_path_and_of_the_product(tmp_path_factory):
    """(2), (3): every instrumented index (the fragment reads' among them) inside its extent, bit-identical |p| with OLX_EXP_CP_NOFILLAHEAD=1; then the
    child's volumes against the product library's where the two run the same products (a forced-e4m3 case differs from the product's fp16 corrections
    by design: its volume meets the oracle in the test below)."""
    code, tail, out = debug_launches(tmp_path_factory)
    assert code == 0, (code, tail)
    assert tail.count("SAME BITS:") == len(NAMES), tail
    compared = 0
    for case in NAMES:
        name, p, _ = product_launch(case)
        dbg = np.load(os.path.join(out, case + ".npy"))
        if F.CASES[case].get("force") and "fp8corr" not in name:
            continue
        assert np.array_equal(dbg, p), case
        compared += 1
    assert compared >= len(NAMES) - 2


FORCED = [c for c in NAMES if F.CASES[c].get("force")]


@pytest.mark.gpu
@pytest.mark.parametrize("case", FORCED)
def test_forced_e4m3_volume_of_the_debug_library_matches_the_oracle(case, tmp_path_factory):
    """(1) for the e4m3 body where the planner may keep it off the grid (ragged nz; the e4m3 + clamp instantiation): the debug library's launch with
    the e4m3 products forced must NAME them, and its full |p| volume of every focus meets the fp64 C oracle (computed from the steering the child
    itself solved) at the gate of a variant that says fp8corr.  The product's launch of these cases (test_volume_matches_the_oracle) may run the fp16
    corrections, and the comparison with the other fill path goes through the same fragment addresses: neither would see a wrong in-range address here."""
    code, tail, out = debug_launches(tmp_path_factory)
    assert code == 0, (code, tail)
    with open(os.path.join(out, case + ".txt")) as fh:
        name = fh.read()
    cs = F.CASES[case]
    assert "field_cosetp_k<nt2" in name and "fp8corr" in name and cs["expect"] in name and "nofillahead" not in name, name
    _, _, (_, pos_m, area, foci, _, _, coords) = product_launch(case)
    steer = np.load(os.path.join(out, case + "_steer.npz"))
    p = np.load(os.path.join(out, case + ".npy"))
    assert len(p) == len(foci) == len(steer["d"])
    worst = worst_error(p, cs, pos_m, area, steer["d"], steer["ap"], coords)
    print(f"{case} (debug library, e4m3 forced): {name.strip()[:90]} | worst |p| error {worst:.3e} of the volume maximum (gate {R.FP8_BOUND:.1e})")
    assert worst <= R.FP8_BOUND, (case, worst)
