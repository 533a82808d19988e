"""Kernel 2g (field_cosetp_k): the steering fragments of a table pair are requested a whole chunk at a time -- ONE block-uniform test per request (none for
the first pair, `sb0 + 2 < n_sb` for the next one), a scalar base per 8 KiB part plus the lane's 32-bit byte offset, and nothing at all (no zero fill)
when there is no next pair.  The host refuses a plan whose super-block count is odd or whose operand sets do not hold n_tiles x n_sb whole super-blocks
(olx.hip).  Arithmetic, LDS layout, barriers and the order of the matrix instructions are the parent's: the bits must not change.

The cases are the ways a request can go wrong, on the small grids of tests/test_gpu_cosetp_tile_addr.py (1 mm grid, 3 mm pitch, KX = 3 / KY = 11 blocks):

  nsa1_8x16              one pair per block: NO request after the first; the loop ends with pre[] unassigned and stages nothing more
  nsa2_16x16             the headline's shape: one request
  nsa3_20x16             two requests
  nsbp4_odd_nsb_16x24    24 element rows: nsb = 3 padded to nsbp = 4 -- the chunk of (sbb 2, padding sbb 3) is requested whole, its padding half holds zero weights
  two_tiles_5foci        20 steering columns in two launch tiles: `tile` offsets the base
  split_two_tiles_nz768  e4m3 products from plane 32 on, fp16 x 3 below (operands bfrag_half on), in two tiles: the smallest volume at which the planner splits
                         a launch of this lateral shape (8e6 (voxel, focus) pairs above the cut: fp8_split_pays)
  fp16_corr              the fp16-correction instantiation (requests in front of the K-steps)
  clamp_e4m3, ragged_nz23_e4m3   the e4m3 + clamp instantiation and a ragged nz; the debug-library child forces the e4m3 products (OLX_FP8_CORRECTION=1), the
                         variant must then say fp8corr
  clamp, absorption_dir  clamp with fp16 corrections; the DIR instantiation
  2e_nt1_e4m3, 2e_nt4_fp16, 2d_nt1_fp16, 2d_nt2_clamp_fp16   kernels 2e and 2d, which request in 8 KiB parts under one uniform test per part: one and four parts
                         per request in 2e (e4m3 / fp16 corrections), NT = 1 and NT = 2 in 2d (complex output: the launches the planner gives it; no e4m3 form exists)

Every case: (1) |p| of the product's launch against the fp64 C oracle at the sibling files' gates (1e-5 of the volume maximum; 7.5e-6 where the variant
says fp8corr) -- the full volume of every focus, except the split launch, whose 1.8 M voxels are checked for every focus on every plane of the first 64 (both
sides of the cut) and every 16th above, against those planes' own maximum (never larger than the volume's: not a wider gate; its full volume is compared
bit by bit with the debug library's) --,
(2) the debug library's |p| bit-identical to the product's wherever both run the same products, (3) an empty bounds report from the debug library, which
checks every lane's entry of every request against the launch tile's own records.  A forced-e4m3 launch of the debug library meets the oracle at 7.5e-6,
the gate of a variant that says fp8corr (tests/test_gpu_cosetp_tile_addr.py).

On the host: the planner's real decision (tools/plan_query.cpp) names the expected kernel, tile count and products for every case, and the case table's
own claims are checked (pairs per block, the padding super-block, the block shape).  The host tests say nothing about the kernel's addresses: those
are covered on the GPU by the oracle, the bit comparison and the bounds report."""
import os
import subprocess
import sys

import numpy as np
import pytest

from openlifu_amd import _native as nat
from oracle import bf_oracle as bo, c_oracle as co

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plan_query as PQ                      # noqa: E402
import test_gpu_cosetp_fill_ahead as F       # noqa: E402  (elements_of, coords_of, the foci inside 23 planes)
import test_gpu_cosetp_table_reuse as R      # noqa: E402  (block_shapes, the foci, the gates)

ROOT = R.ROOT
F0, C, RHO, P0 = R.F0, R.C, R.RHO, R.P0
TOL_P, FP8_BOUND = R.TOL_P, R.FP8_BOUND
FOCI5 = R.FOCI9[:5]                           # 5 foci x 4 mirror images = 20 columns: two launch tiles of 16
FOCI5_IN = [[1e-3, 2e-3, 16e-3], [-3e-3, 1e-3, 14e-3], [2e-3, -4e-3, 12e-3], [-2e-3, -3e-3, 18e-3], [4e-3, 1e-3, 15e-3]]      # inside 16 planes from z = 5 mm
FOCI5_DEEP = [[1e-3, 2e-3, 60e-3], [-3e-3, 1e-3, 56e-3], [2e-3, -4e-3, 52e-3], [-2e-3, -3e-3, 64e-3], [4e-3, 1e-3, 58e-3]]
G = (36, 64, 32)

# e4m3: True / False = the product's variant must (not) say fp8corr; force = the debug-library child pins OLX_FP8_CORRECTION=1; tiles = launch tiles;
# oz = planes the oracle is evaluated on (default: all); kern = the kernel the planner must name (default: 2g)
CASES = {
    "nsa1_8x16":             dict(arr=(8, 16), n=G, e4m3=False, force=True, expect="mx2,my2,flat,noclamp", nsa=1, nsbp=2, tiles=1),
    "nsa2_16x16":            dict(arr=(16, 16), n=G, e4m3=True, expect="mx2,my2,flat,noclamp", nsa=2, nsbp=2, tiles=1),
    "nsa3_20x16":            dict(arr=(20, 16), n=G, e4m3=True, expect="mx2,my2,flat,noclamp", nsa=3, nsbp=2, tiles=1),
    "nsbp4_odd_nsb_16x24":   dict(arr=(16, 24), n=G, e4m3=True, expect="mx2,my2,flat,noclamp", nsa=2, nsbp=4, tiles=1),
    "two_tiles_5foci":       dict(arr=(16, 16), n=G, e4m3=True, foci=FOCI5, expect="mx2,my2,flat,noclamp", frag="20 columns for 5 foci x 4 images in 2 tile(s)", nsa=2, nsbp=2, tiles=2),
    "split_two_tiles_nz768": dict(arr=(16, 16), n=(36, 64, 768), e4m3=True, foci=FOCI5_DEEP, z0=-4e-3, expect="mx2,my2,flat,clamp,fp8corr from plane 32>",
                                  frag="in 2 tile(s)", nsa=2, nsbp=2, tiles=2, oz=list(range(64)) + list(range(64, 768, 16))),
    "fp16_corr":             dict(arr=(16, 16), n=G, e4m3=False, fp16=True, expect="mx2,my2,flat,noclamp", nsa=2, nsbp=2, tiles=1),
    "clamp_e4m3":            dict(arr=(16, 16), n=G, e4m3=False, force=True, foci=F.FOCI_IN, z0=-4e-3, expect="flat,clamp", nsa=2, nsbp=2, tiles=1),
    "ragged_nz23_e4m3":      dict(arr=(16, 16), n=(36, 64, 23), e4m3=True, force=True, foci=F.FOCI_IN, expect="mx2,my2,flat,noclamp", nsa=2, nsbp=2, tiles=1),
    "clamp":                 dict(arr=(16, 16), n=G, e4m3=False, z0=-4e-3, expect="flat,clamp", nsa=2, nsbp=2, tiles=1),
    "absorption_dir":        dict(arr=(16, 16), n=G, e4m3=False, absorb=40.0, expect="uniform absorption", nsa=2, nsbp=2, tiles=1),
    # kernels 2e and 2d request in parts of 8 KiB, NT parts per super-block (k_coset.hip, k_lattice.hip): the rows of tests/test_gpu_lattice_matrix.py on their
    # smallest grids.  2e: one part per request with e4m3 products (NT = 1), four with fp16 (NT = 4); 2d (complex output; it has no e4m3 instantiation):
    # NT = 1 and NT = 2 with the clamp, both fp16
    "2e_nt1_e4m3":           dict(kern="field_coset_k<nt1", arr=(16, 16), n=G, e4m3=True, foci=R.FOCI3[:2], expect="mx2,my2,flat,noclamp,fp8corr>", frag="8 columns", nsa=2, nsbp=2, tiles=1),
    "2e_nt4_fp16":           dict(kern="field_coset_k<nt4", arr=(16, 16), n=(36, 40, 16), e4m3=False, fp16=True, foci=FOCI5_IN, expect="mx2,my2,flat,noclamp>",
                                  frag="20 columns for 5 foci x 4 images in 1 tile(s)", nsa=2, nsbp=2, tiles=1),
    "2d_nt1_fp16":           dict(kern="field_lattice_k<mt4,nt1", arr=(8, 16), n=(25, 28, 9), e4m3=False, cplx=True, foci=R.FOCI3[:2], expect="mx2,my2,flat,noclamp>", nsa=1, nsbp=2, tiles=1),
    "2d_nt2_clamp_fp16":     dict(kern="field_lattice_k<mt4,nt2", arr=(8, 16), n=(25, 28, 9), e4m3=False, cplx=True, z0=-4e-3, expect="mx2,my2,flat,clamp>", nsa=1, nsbp=2, tiles=1),
}
KERN_2G = "field_cosetp_k<nt2"
K2G = [c for c in CASES if "kern" not in CASES[c]]
NAMES = list(CASES)

def steering_of(cs):
    pos_m, area = F.elements_of(cs)
    foci = np.asarray(cs.get("foci", R.FOCI3))
    st = [bo.beamform(pos_m, np.zeros_like(pos_m), f, C) for f in foci]
    return pos_m, area, foci, np.array([s[0] for s in st]), np.array([s[1] for s in st])


# ---- host tests (no GPU) ----
def test_the_case_table_has_the_pairs_tiles_and_block_shapes_claimed_for_it():
    seen = set()
    for name, cs in CASES.items():
        nax, nay = cs["arr"]
        nsa, nsb = (nax + 7) // 8, (nay + 7) // 8
        assert (nsa, (nsb + 1) & ~1) == (cs["nsa"], cs["nsbp"]), name
        if name in K2G:
            seen.add((cs["nsa"] * cs["nsbp"] // 2 - 1, cs["tiles"]))      # requests after the first one, launch tiles
            shapes = R.block_shapes(cs["n"], (True, True))
            assert (3, 11) in shapes and max(a * b for a, b in shapes) == 33, name
    # no request, one, two (and three: nsbp = 4) after the first; one and two tiles
    assert {(0, 1), (1, 1), (2, 1), (3, 1), (1, 2)} <= seen, seen
    # the padding super-block: 24 element rows are 3 super-block rows in 4 slots
    assert (CASES["nsbp4_odd_nsb_16x24"]["arr"][1] + 7) // 8 == 3


def test_the_real_planner_names_the_expected_variant_for_every_case():
    """olxplan::decide_variant through tools/plan_query.cpp: kernel 2g, the tile count, the correction products of the product library -- and fp8corr
    under the developer pin for the forced cases."""
    for name, cs in CASES.items():
        pos_m, area, foci, d, ap = steering_of(cs)
        xs, ys, zs = F.coords_of(cs)
        v = PQ.variant(pos_m, area, d, ap, xs, ys, zs, F0, C, RHO, P0, ("pmag", "complex") if cs.get("cplx") else ("pmag",), foci=foci, fp16=cs.get("fp16", False),
                       absorb=cs.get("absorb", 0.0))
        assert cs.get("kern", KERN_2G) in v and cs["expect"] in v and cs.get("frag", "") in v, (name, v)
        assert ("fp8corr" in v) == cs["e4m3"], (name, v)
        assert f"in {cs['tiles']} tile(s)" in v, (name, v)
        if cs.get("force"):
            v = PQ.variant(pos_m, area, d, ap, xs, ys, zs, F0, C, RHO, P0, ("pmag",), foci=foci, fp8_pin="1", dev=True)
            assert KERN_2G in v and "fp8corr>" in v and f"in {cs['tiles']} tile(s)" in v, (name, v)
    # the split: two operand sets, the cut on a plane-block boundary with at least three quarters of the planes above it
    assert 4 * 32 <= CASES["split_two_tiles_nz768"]["n"][2]


# ---- GPU ----
def prepare(ctx, name):
    """Elements, steering (kernel 1 on the device: the library then knows the foci) and the grid of a case."""
    cs = CASES[name]
    pos_m, area = F.elements_of(cs)
    ctx.set_elements(pos_m, np.tile([0.0, 0.0, 1.0], (len(pos_m), 1)), area)
    foci = np.asarray(cs.get("foci", R.FOCI3))
    d, ap = ctx.bf_solve(foci, C)
    ctx.field_absorption(cs.get("absorb", 0.0))
    return cs, pos_m, area, foci, d, ap, F.coords_of(cs)


def launch(ctx, cs, coords):
    """Plan and launch (|p| alone: the product's outputs; with the complex field for kernel 2d); returns the variant name and the |p| volumes [focus]."""
    xs, ys, zs = coords
    flags = nat.OUT_PMAG | (nat.OUT_COMPLEX if cs.get("cplx") else 0) | (nat.FIELD_FP16_CORRECTION if cs.get("fp16") else 0)
    ctx.field_plan((xs[0], ys[0], zs[0]), (1e-3,) * 3, cs["n"], F0, C, RHO, P0, flags=flags)
    name = ctx.field_variant()
    assert cs.get("kern", KERN_2G) in name and f"in {cs['tiles']} tile(s)" in name, name
    ctx.field_launch()
    return name, ctx.field_fetch_all(want=("pmag",))["pmag"]


_PRODUCT = {}


def product_launch(case):
    """The product library's launch of a case, once per session: (variant name, |p| [focus], inputs of the oracle)."""
    if case not in _PRODUCT:
        ctx = nat.Context(0)
        try:
            cs, pos_m, area, foci, d, ap, coords = prepare(ctx, case)
            name, p = launch(ctx, cs, coords)
            ctx.field_absorption(0.0)
        finally:
            ctx.close()
        _PRODUCT[case] = (name, p, (cs, pos_m, area, foci, d, ap, coords))
    return _PRODUCT[case]


def worst_error(p, cs, pos_m, area, d, ap, coords):
    """Largest |p| error over the checked planes of the checked foci against the fp64 C oracle, as a share of each reference's maximum."""
    xs, ys, zs = coords
    oz = np.asarray(cs.get("oz", range(len(zs))))
    worst = 0.0
    for f in range(len(d)):
        ref = np.abs(co.field_on_grid(xs, ys, zs[oz], pos_m, area, d[f], ap[f], F0, C, P0, dmin=0.5e-3, absorption=cs.get("absorb", 0.0)))
        got = np.asarray(p[f]).reshape(len(xs), len(ys), len(zs))[:, :, oz]
        assert np.isfinite(got).all() and ref.max() > 0
        worst = max(worst, np.abs(got - ref).max() / ref.max())
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("case", NAMES)
def test_volume_matches_the_oracle(case):
    """(1) |p| of every checked focus against the fp64 C oracle with the product's launch."""
    name, p, (cs, pos_m, area, foci, d, ap, coords) = product_launch(case)
    assert cs["expect"] in name and cs.get("frag", "") in name, name
    assert ("fp8corr" in name) == cs["e4m3"], name
    tol = FP8_BOUND if "fp8corr" in name else TOL_P
    worst = worst_error(p, cs, pos_m, area, d, ap, coords)
    print(f"{case}: {name.strip()[:100]} | worst |p| error {worst:.3e} of the maximum (gate {tol:.1e})")
    assert worst <= tol, (case, worst)


_CHILD = r"""
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
from openlifu_amd import _native as nat
import test_gpu_cosetp_steer_request as T
out = %r
assert "libolx_dbg" in os.path.basename(nat.LIB_PATH), nat.LIB_PATH
for case in T.NAMES:
    ctx = nat.Context(0)
    cs, pos_m, area, foci, d, ap, coords = T.prepare(ctx, case)
    os.environ.pop("OLX_FP8_CORRECTION", None)
    name, p = T.launch(ctx, cs, coords)
    ctx.sync()          # the debug library reports accesses outside their extent here
    if not (np.isfinite(p).all() and p.max() > 0):
        print("NOT FINITE:", case, name)
        sys.exit(3)
    np.save(os.path.join(out, case + ".npy"), p)
    with open(os.path.join(out, case + ".txt"), "w") as fh:
        fh.write(name)
    if cs.get("force"):
        os.environ["OLX_FP8_CORRECTION"] = "1"
        name8, p8 = T.launch(ctx, cs, coords)
        os.environ.pop("OLX_FP8_CORRECTION", None)
        ctx.sync()
        assert "fp8corr" in name8, name8
        np.save(os.path.join(out, case + "_forced.npy"), p8)
        np.savez(os.path.join(out, case + "_steer.npz"), d=d, ap=ap)
        with open(os.path.join(out, case + "_forced.txt"), "w") as fh:
            fh.write(name8)
    ctx.close()
    print("INSIDE:", case, "|", name.strip()[:70])
sys.exit(0)
"""

_DEBUG = {}


def debug_launches(tmp_path_factory):
    """All cases in ONE child process on lib/libolx_dbg.so, once per session: (return code, end of the output, directory of the volumes it saved)."""
    if not _DEBUG:
        out = str(tmp_path_factory.mktemp("steer_request_dbg"))
        lib = os.path.join(ROOT, "openlifu-python_amd", "lib", "libolx_dbg.so")
        env = dict(os.environ, OLX_LIB_PATH=lib)
        for k in ("OLX_FIELD_VARIANT", "OLX_FP8_CORRECTION", "OLX_EXP_KGRP", "OLX_INTENSITY_STORED", "OLX_EXP_CP_NOREUSE", F.PIN):
            env.pop(k, None)
        code = _CHILD % (ROOT, os.path.join(ROOT, "openlifu-python_amd"), os.path.join(ROOT, "tests"), out)
        r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
        _DEBUG["run"] = (r.returncode, (r.stdout + r.stderr)[-3000:], out)
    return _DEBUG["run"]


@pytest.mark.gpu
def test_debug_library_reports_nothing_and_has_the_bits_of_the_product(tmp_path_factory):
    """(2), (3): every lane's entry of every request (and every other instrumented index) inside its extent; the debug library's |p| bit-identical to the
    product library's -- the debug library plans the same products without the pin, so every case is compared."""
    code, tail, out = debug_launches(tmp_path_factory)
    assert code == 0, (code, tail)
    assert tail.count("INSIDE:") == len(NAMES), tail
    for case in NAMES:
        name, p, _ = product_launch(case)
        with open(os.path.join(out, case + ".txt")) as fh:
            dname = fh.read()
        assert dname.split(";")[0] == name.split(";")[0], (case, dname, name)
        assert np.array_equal(np.load(os.path.join(out, case + ".npy")), p), case


FORCED = [c for c in NAMES if CASES[c].get("force")]


@pytest.mark.gpu
@pytest.mark.parametrize("case", FORCED)
def test_forced_e4m3_volume_of_the_debug_library_matches_the_oracle(case, tmp_path_factory):
    """The e4m3 body where the product's planner keeps the fp16 corrections (one pair per block; the e4m3 + clamp instantiation) and on a ragged nz: the
    debug library's forced launch must NAME the e4m3 products, and its full |p| volume meets the fp64 C oracle (computed from the steering the child itself
    solved) at 7.5e-6, the gate of a variant that says fp8corr."""
    code, tail, out = debug_launches(tmp_path_factory)
    assert code == 0, (code, tail)
    with open(os.path.join(out, case + "_forced.txt")) as fh:
        name = fh.read()
    cs = CASES[case]
    assert KERN_2G in name and "fp8corr" in name and cs["expect"] in name, name
    _, _, (_, pos_m, area, foci, _, _, coords) = product_launch(case)
    steer = np.load(os.path.join(out, case + "_steer.npz"))
    p = np.load(os.path.join(out, case + "_forced.npy"))
    assert len(p) == len(foci) == len(steer["d"])
    tol = FP8_BOUND
    worst = worst_error(p, cs, pos_m, area, steer["d"], steer["ap"], coords)
    print(f"{case} (debug library, e4m3 forced): {name.strip()[:90]} | worst |p| error {worst:.3e} of the volume maximum (gate {tol:.1e})")
    assert worst <= tol, (case, worst)
