"""Parity matrix of the lattice field kernels -- 2d (field_lattice_k), 2e (field_coset_k), 2g (field_cosetp_k), 2f (field_toep_k) -- against the
fp64 C oracle, modelled on tests/test_gpu_field_matrix.py (kernels 2a / 2b / 2c).

Every array here is a flat matrix array whose pitch is a whole number of voxels, so the planner (decide_variant in olx_plan.cpp) has to
choose among the ~ 180 instantiations of these four kernels from the mirror folds of the geometry, the number of distinct steering vectors, the output
set, the arithmetic of the correction products, per-term modifiers and the pins.  One table (CASES) names for every case the instantiation it must
reach -- the string olx_field_variant reports up to '>', and where it matters a later fragment ("in 2 tile(s)", "3 row tile(s)", "piston directivity
in the tables") -- and the full planned volume of every requested output is compared with oracle.c_oracle.field_on_grid at the project's gates
(|p| 1e-5, complex 3e-5, intensity 2e-5 of the reference maximum; dmin = half the smallest spacing); a variant that says fp8corr also keeps the
7.5e-6 that include/olx.h promises.  The planner exits (poor fills, NT = 4 with complex output, a pitch that is no whole number of voxels, too much
padding, one rolled element under the directivity flag) have rows of their own with the string of the kernel that takes over.

Fold patterns come from the geometry, never from a pin: grid centred on the array = both folds, shifted by whole voxels along one axis = the other
fold only, shifted along both = none, an x-slab of a centred grid = the y fold only.

Tests without a GPU: the coverage test (the table's strings reach every instantiation and shape edge the matrix is for, the size caps), the decision test
(the REAL decision, olxplan::decide_variant asked through tools/plan_query.cpp, produces every row's expected string and fragments, and agrees with
plan_rule on every row), the rule test (the planner's decision restated independently in plan_rule predicts every expected string; lattice detection
with its clamp bound, column packing, coset_tiles16, toep_plan and the e4m3 rule are ASKED of the real olx_plan.cpp, not restated a third time), the oracle alone and the
sensitivity test (a dropped element row, an array displaced by one pitch and a mirrored store target each move the reference by more than ten gates).

Left out on purpose: split launches ("fp8corr from plane K").  fp8_split_pays needs >= 8e6 (voxel, focus) pairs above the cut, i.e. more than 2e9
oracle terms at 256 elements; test_e4m3_rule_near_the_array and test_split_launch_with_several_column_tiles_and_in_a_slab (test_gpu_field.py) keep that ground.

Instantiations the product's planner does not reach at the 256-element shapes of this table, read from the planner: e4m3 corrections together
with clamp.  The clamp tag needs a voxel closer than one spacing to a (real or virtual) lattice point, i.e. a grid through or right above the element
plane; fp8_first_plane then admits the e4m3 products only from a later plane block on, and fp8_split_pays refuses the split below 8e6 (voxel, focus)
pairs, so the launch keeps fp16 corrections.  (One product row does have both: 2f-y-xaxis-focus-clamp, 320 elements focused 12 mm deep, where the
focal peak outweighs the near-field sum.)  The other instantiations (2e / 2g / 2f NM = 1 .. 3 with clamp,fp8corr) are in DEV_CASES: they need
OLX_FP8_CORRECTION=1, which only a developer build honours, and run in the debug-library child of tests/test_gpu_debug_bounds.py.  The pin forces the e4m3 products PAST the rule that makes
the 7.5e-6 promise, so those cases are held to the project's gates only."""
import ctypes
import functools
import re

import numpy as np
import pytest

from openlifu_amd import _native as nat
from oracle import bf_oracle as bo, c_oracle as co, field_oracle as fo
from plan_query import _d, _i, planq, variant as real_variant_of      # the real planning code (olx_plan.cpp) behind a C interface
from test_gpu_field import C, DEV_LIB, F0, FP8_BOUND, P0, RHO, TOL_I, TOL_P, setup_ctx
from test_gpu_field_matrix import APODS, FOLDS, OUTPUTS, distance_class, measure
from test_gpu_cosetp_table_reuse import block_shapes

GATES = {"pmag": TOL_P, "complex": 3 * TOL_P, "intensity": TOL_I}
CAP, CAP_BIG, MAX_BIG = 2e8, 6e8, 4      # oracle terms (voxels x elements x foci) per case; the named exceptions are the NM = 3 cases of kernel 2f
SHIFT = (3, -2)                          # whole voxels: the shift that takes a fold away
SWEEP_SEED, SWEEP_DRAWS = 20262, 12
APODS = [APODS[0], ("maxangle", 45.0, 0.0), APODS[2]]      # (45 degrees: at the 30 mm the angle-limited foci sit at, the outer rows keep weight and only corners are silent)
ABSORB = 40.0                            # Np/m (tissue-like at 400 kHz)


# ---- geometry ------------------------------------------------------------------------------------------------------------------------------------
def geometry(case):
    """positions [mm] (element e = a * nay + b), orientations [rad], sizes [mm]; grid coordinate vectors [m]."""
    nax, nay = case["arr"]
    h = case["h"]
    px, py = case["pitch"][0] * h[0], case["pitch"][1] * h[1]
    a, b = np.meshgrid(np.arange(nax), np.arange(nay), indexing="ij")
    pos = np.stack([(a.ravel() - (nax - 1) / 2) * px, (b.ravel() - (nay - 1) / 2) * py, np.zeros(nax * nay)], axis=1)
    ori = np.zeros_like(pos)
    if case.get("rolled"):
        ori[37 % len(pos), 2] = 0.2                                       # one element rolled about its normal: its frame differs from the others'
    size = np.tile([0.9 * px, 0.9 * py], (len(pos), 1))
    nx, ny, nz = case["n"]
    sx, sy = case["shift"]
    xs = ((np.arange(nx) - (nx - 1) / 2) + sx) * h[0]; ys = ((np.arange(ny) - (ny - 1) / 2) + sy) * h[1]
    zs = case["z0"] + np.arange(nz) * h[2]
    return pos, ori, size, xs * 1e-3, ys * 1e-3, zs * 1e-3


def _foci(kind, F, case, seed):
    nz = case["n"][2]
    zlo, dz = case["z0"], (nz - 1) * case["h"][2]
    k = np.arange(F)
    zk = zlo + dz * (0.55 + 0.35 * ((k * 0.37) % 1.0))                    # inside the planes (the e4m3 rule asks for that), distinct
    zk = np.where(zk < 12.0, 12.0 + 0.4 * k, zk)                          # ... and never next to the element plane (shallow grids, grids through the plane)
    if case["apod"][0] != "uniform":
        zk = 30.0 + 1.7 * k       # angle-limited drive: deep enough that the outermost element row still carries weight (only its corners are silent)
    if kind == "wheel":
        return np.roll(bo.wheel_targets([0, 0, max(zlo + 0.7 * dz, 12.0)], True, F - 1, 4.0), -1, axis=0)      # (the on-axis target last: focus 0 has distinct images)
    if kind == "generic":
        rng = np.random.default_rng(seed + 131 * F)
        xy = rng.uniform(0.6, 4.0, (F, 2)) * rng.choice([-1.0, 1.0], (F, 2))
        return np.column_stack([xy, zk])
    off = 0.9 + 0.7 * k * (-1.0) ** k
    zero = np.zeros(F)
    return np.column_stack([off if kind == "xaxis" else zero, off if kind == "yaxis" else zero, zk])


def foci_of(case):
    """[F, 3] m.  ("generic", F): off both symmetry planes; "axis": on the array's axis (all images share one steering vector); "xaxis" / "yaxis": on
    that axis (the images of the other fold coincide); "wheel": a Wheel of F - 1 spokes around the axis (mirror-partner foci); a tuple of such pairs
    is their concatenation."""
    spec = case["foci"]
    if isinstance(spec[0], str):
        spec = (spec,)
    return np.concatenate([_foci(kind, F, case, case.get("seed", 7) + 17 * q) for q, (kind, F) in enumerate(spec)]) * 1e-3


def steering(case):
    pos, ori, _, *_ = geometry(case)
    st = [bo.beamform(pos * 1e-3, ori, f, C, apod=case["apod"]) for f in foci_of(case)]
    return np.array([s[0] for s in st]), np.array([s[1] for s in st])


def modifiers(case):
    """(directivity triple or None, absorption [Np/m]) as c_oracle.field_on_grid takes them."""
    pos, ori, size, *_ = geometry(case)
    R = bo.element_rotations(ori)
    return ((R[:, :, 0], R[:, :, 2], size * 1e-3) if case["dirv"] else None), case["absorb"]


def n_terms(case):
    return float(np.prod(case["n"])) * case["arr"][0] * case["arr"][1] * len(foci_of(case))


# ---- the case table --------------------------------------------------------------------------------------------------------------------------------
def _case(kern, arr, pitch, n, folds="xy", clamp=False, nt=None, e4m3=False, foci=("generic", 3), out="p", frag=(), **kw):
    """One row.  kern / nt / folds / clamp / e4m3 are WRITTEN here (they make `want`); plan_rule derives them again from the geometry."""
    c = dict(kern=kern, arr=arr, pitch=pitch, n=n, h=(1.0, 1.0, 1.0), z0=None, slab=None, foci=foci, apod=APODS[0], out=out, pin=None, stored=False, dirv=False,
             absorb=0.0, fp16=False, e4m3=e4m3, rolled=False, dev=False, frag=tuple(frag), folds=folds)
    c.update(kw)
    if isinstance(c["apod"], int):
        c["apod"] = APODS[c["apod"]]
    if c["z0"] is None:
        c["z0"] = -4.0 * c["h"][2] if clamp else 5.0
    c["shift"] = kw.get("shift", (0 if "x" in folds or c["slab"] else SHIFT[0], 0 if "y" in folds else SHIFT[1]))
    mx, my = FOLDS[folds]
    if c["slab"]:
        mx = 1
    cl = "clamp" if clamp else "noclamp"
    f8 = ",fp8corr" if e4m3 else ""
    c["want"] = {"2g": f"field_cosetp_k<nt2,mx{mx},my{my},flat,{cl}{f8}>", "2e": f"field_coset_k<nt{nt},mx{mx},my{my},flat,{cl}{f8}>",
                 "2d": f"field_lattice_k<mt4,nt{nt},mx{mx},my{my},flat,{cl}>", "2f": f"field_toep_k<mx{mx},my{my},flat,{cl}{f8}>",
                 "2c": f"field_mfma_k<mt{4 if n[2] >= 48 else 1},nt{nt},mx{mx},my{my},flat,{cl}>", "dir": f"field_accum_dir_k<4,{cl}>"}[kern]
    return c


A16, A8x16, A20x16, A16x32, A20x12, A9x23, A16x20, A12x16, A18x16 = (16, 16), (8, 16), (20, 16), (16, 32), (20, 12), (9, 23), (16, 20), (12, 16), (18, 16)
P3 = (3, 3)
G_BASE = (36, 64, 32)       # the admitted e4m3 shape: 16 x 16 uniformly driven, 1 mm, z from 5 mm; KX = 3 x KY = 11 blocks (test_gpu_cosetp_table_reuse.py)
# columns per fold pattern: NT = 2 needs 9 .. 16 of them, NT = 1 2 .. 8, NT = 4 17 .. 32; a generic focus makes one column per mirror image
NF2 = {"xy": 3, "x": 5, "y": 5, "": 9}
NF1 = {"xy": 2, "x": 3, "y": 4, "": 7}
NF4 = {"xy": 5, "x": 9, "y": 10, "": 17}


def _build_cases():
    cs = {}
    # ---- kernel 2g: folds 4 x clamp 2 x {fp16, e4m3 corrections}; clamp + e4m3 needs the developer pin (module docstring)
    g_fp16 = {"xy": (A8x16, (40, 44, 23), P3, 1), "x": (A20x12, (30, 50, 20), P3, 2), "y": (A16x20, (36, 40, 17), (3, 2), 1), "": (A9x23, (31, 45, 16), (4, 2), 2)}
    for folds in FOLDS:
        F = NF2[folds]
        small = (36, 40, 16) if folds == "" else G_BASE
        cs[f"2g-{folds or 'none'}-e4m3"] = _case("2g", A16, P3, small, folds, e4m3=True, foci=("generic", F))
        arr, n, pitch, ap = g_fp16[folds]
        cs[f"2g-{folds or 'none'}-fp16"] = _case("2g", arr, pitch, n, folds, foci=("generic", F), apod=ap, out="pi")
        cs[f"2g-{folds or 'none'}-clamp"] = _case("2g", A12x16 if folds == "xy" else arr, pitch, (60, 40, 17) if folds == "xy" else n, folds, clamp=True, foci=("generic", F), apod=ap)
        cs[f"2g-{folds or 'none'}-clamp-e4m3-dev"] = _case("2g", A16, P3, (36, 40, 16), folds, clamp=True, e4m3=True, foci=("generic", F), dev=True, z0=0.75)
    cs["2g-xy-fp16-flag"] = _case("2g", A16, P3, G_BASE, "xy", fp16=True)                                               # the opt-out flag on the admitted shape
    # the three epilogues, each with nz % 4 == 0 and with a ragged nz (kernel 2g, and 2e NT = 1 for the bit-identity test)
    for nz in (32, 23):
        for out, stored in (("p", False), ("pi", True), ("i", True)):
            cs[f"2g-epi-{out}{'-stored' if stored else ''}-nz{nz}"] = _case("2g", A16, P3, (36, 64, nz), "xy", e4m3=True, foci=("generic", 3), out=out, stored=stored)
            cs[f"2e-epi-{out}{'-stored' if stored else ''}-nz{nz}"] = _case("2e", A8x16, P3, (36, 44, nz), "xy", nt=1, foci=("generic", 2), out=out, stored=stored, apod=1)
    # DIR instantiations of 2g: two fold patterns, both clamp values
    cs["2g-xy-dir-piston"] = _case("2g", A8x16, P3, (40, 44, 24), "xy", dirv=True, apod=1, out="pi", frag=("piston directivity in the tables",))
    cs["2g-x-dir-absorb-clamp"] = _case("2g", A20x12, P3, (30, 50, 20), "x", clamp=True, foci=("generic", 5), absorb=ABSORB, frag=("uniform absorption in the tables",))
    cs["2g-y-dir-both"] = _case("2g", A16x20, (3, 2), (36, 40, 17), "y", foci=("generic", 5), dirv=True, absorb=ABSORB, frag=("piston directivity in the tables", "uniform absorption in the tables"))
    cs["2g-none-dir-piston-clamp"] = _case("2g", A9x23, (4, 2), (31, 45, 16), "", clamp=True, foci=("generic", 9), dirv=True, frag=("piston directivity in the tables",))
    # element counts of test_gpu_cosetp_table_reuse.py (nsa = 1 / 2 / 3, nsbp = 4) -- 16 x 16 is above
    cs["2g-nsa1-8x16"] = _case("2g", A8x16, P3, G_BASE, "xy", apod=2)
    cs["2g-nsa3-20x16"] = _case("2g", A20x16, P3, (36, 64, 16), "xy", e4m3=True)
    cs["2g-nsbp4-16x32"] = _case("2g", A16x32, P3, (36, 40, 16), "xy", e4m3=True)
    # column tiles: 36 columns in three 16-column tiles; 20 columns cut in two where the e4m3 rule applies; shared and balanced columns
    cs["2g-xy-36col-3tiles"] = _case("2g", A8x16, P3, (36, 44, 17), "xy", foci=("generic", 9), apod=1, frag=("36 columns for 9 foci x 4 images in 3 tile(s)",))
    cs["2g-xy-20col-e4m3-2tiles"] = _case("2g", A16, P3, (36, 40, 16), "xy", e4m3=True, foci=("generic", 5), frag=("20 columns for 5 foci x 4 images in 2 tile(s)",))
    cs["2g-xy-wheel-shared"] = _case("2g", A8x16, P3, (36, 44, 17), "xy", foci=("wheel", 8), out="pi")
    cs["2g-xy-onaxis-balanced"] = _case("2g", A8x16, (3, 2), (41, 44, 37), "xy", foci=(("generic", 2), ("axis", 2)), frag=("10 columns for 4 foci x 4 images",))
    cs["2g-x-16col-aniso"] = _case("2g", A20x12, (2, 5), (33, 50, 20), "x", foci=("generic", 8), h=(1.0, 0.8, 1.25), apod=2, frag=("16 columns",))
    cs["2g-y-9col-pitch1x4"] = _case("2g", A16x20, (1, 4), (24, 60, 16), "y", foci=(("generic", 4), ("xaxis", 1)), apod=2, frag=("9 columns",))
    cs["2g-xy-odd-ny"] = _case("2g", A8x16, P3, (37, 45, 17), "xy", apod=1, out="pi")                                     # the centre row and column are their own mirror images
    cs["2g-xy-above-plane"] = _case("2g", A8x16, P3, (36, 44, 17), "xy", clamp=False, z0=1.0, apod=1)                     # one voxel above the element plane
    # ---- kernel 2e
    e_geo = {"xy": (A8x16, (40, 44, 24), P3), "x": (A20x12, (30, 50, 20), P3), "y": (A16x20, (36, 40, 17), (3, 2)), "": (A9x23, (31, 45, 16), (4, 2))}
    for folds in FOLDS:
        arr, n, pitch = e_geo[folds]
        tag = folds or "none"
        cs[f"2e-nt1-{tag}"] = _case("2e", arr, pitch, n, folds, nt=1, foci=("generic", NF1[folds]), apod=1, out="pi")
        cs[f"2e-nt1-{tag}-clamp"] = _case("2e", arr, pitch, n, folds, clamp=True, nt=1, foci=("generic", NF1[folds]), apod=2)
        cs[f"2e-nt4-{tag}"] = _case("2e", A8x16, P3, (40, 44, 16) if folds == "xy" else (30, 44, 16), folds, nt=4, foci=("generic", NF4[folds]), apod=1, out="pi" if folds == "xy" else "p")
        cs[f"2e-nt2-{tag}-pin"] = _case("2e", arr, pitch, n, folds, nt=2, foci=("generic", NF2[folds]), pin="lattice", apod=2)
    cs["2e-nt4-xy-clamp"] = _case("2e", A8x16, P3, (40, 44, 17), "xy", clamp=True, nt=4, foci=("generic", 8), apod=1, frag=("32 columns",))
    cs["2e-nt4-xy-17col"] = _case("2e", A8x16, P3, (40, 44, 16), "xy", nt=4, foci=(("generic", 4), ("axis", 1)), apod=2, frag=("17 columns",))
    cs["2e-nt4-xy-fp16-flag"] = _case("2e", A16, P3, (36, 40, 16), "xy", nt=4, foci=("generic", 5), fp16=True, frag=("20 columns for 5 foci x 4 images in 1 tile(s)",))
    cs["2e-nt2-xy-clamp-pin"] = _case("2e", A8x16, P3, (40, 44, 17), "xy", clamp=True, nt=2, pin="lattice", out="pi")
    cs["2e-nt1-xy-1col-pin"] = _case("2e", A8x16, P3, (40, 44, 24), "xy", nt=1, foci=("axis", 1), pin="lattice", frag=("1 columns for 1 foci x 4 images",))
    cs["2e-nt1-xy-2col"] = _case("2e", A8x16, P3, (41, 44, 17), "xy", nt=1, foci=("xaxis", 1), apod=1, frag=("2 columns",))
    cs["2e-nt1-xy-e4m3"] = _case("2e", A16, P3, G_BASE, "xy", nt=1, e4m3=True, foci=("generic", 2), frag=("8 columns",))
    cs["2e-nt1-none-e4m3"] = _case("2e", A16, P3, (36, 40, 16), "", nt=1, e4m3=True, foci=("generic", 7))
    cs["2e-nt2-xy-e4m3-pin"] = _case("2e", A16, P3, G_BASE, "xy", nt=2, e4m3=True, pin="lattice")
    cs["2e-nt2-y-e4m3-pin"] = _case("2e", A16, P3, (36, 40, 16), "y", nt=2, e4m3=True, foci=("generic", 5), pin="lattice")
    cs["2e-nt1-xy-clamp-e4m3-dev"] = _case("2e", A16, P3, (36, 40, 16), "xy", clamp=True, nt=1, e4m3=True, foci=("generic", 2), dev=True, z0=0.75)
    cs["2e-nt2-x-clamp-e4m3-dev"] = _case("2e", A16, P3, (36, 40, 16), "x", clamp=True, nt=2, e4m3=True, foci=("generic", 5), dev=True, pin="lattice", z0=0.75)
    cs["2e-nt1-xy-dir-piston"] = _case("2e", A8x16, P3, (40, 44, 24), "xy", nt=1, foci=("generic", 2), dirv=True, apod=1, out="pi", frag=("piston directivity in the tables",))
    cs["2e-nt1-x-dir-absorb"] = _case("2e", A20x12, P3, (30, 50, 20), "x", nt=1, foci=("generic", 3), absorb=ABSORB, frag=("uniform absorption in the tables",))
    cs["2e-nt4-xy-dir-both-clamp"] = _case("2e", A8x16, P3, (40, 44, 17), "xy", clamp=True, nt=4, foci=("generic", 6), dirv=True, absorb=ABSORB, apod=1,
                                           frag=("piston directivity in the tables", "uniform absorption in the tables"))
    cs["2e-nt2-none-dir-piston-pin"] = _case("2e", A9x23, (4, 2), (31, 45, 16), "", nt=2, foci=("generic", 9), dirv=True, pin="lattice", frag=("piston directivity in the tables",))
    cs["2e-nt1-xy-pitch1-unequal-parts"] = _case("2e", A16, (1, 2), (30, 50, 16), "xy", nt=1, foci=("generic", 2), apod=2)       # 8 positions of a coset along x (> 6), 13 along y (> 11)
    cs["2e-nt4-xy-pitch2-unequal-parts"] = _case("2e", A16x20, (2, 1), (26, 30, 16), "xy", nt=4, foci=("generic", 5), apod=1)    # 4 positions along x (> 2), 15 along y
    cs["2e-nt1-xy-aniso-pitch5x2"] = _case("2e", A20x12, (5, 2), (45, 37, 23), "xy", nt=1, foci=("generic", 2), h=(0.6, 1.0, 0.8), apod=1, out="pi")
    # ---- kernel 2d: complex output (NT = 1 / 2), NT = 4 under the lattice2d pin, every fold pattern, both clamp values, nz = 8 / 9
    d_geo = {"xy": (A8x16, (25, 28, 9), P3), "x": (A20x12, (24, 27, 8), P3), "y": (A16x20, (25, 26, 17), (3, 2)), "": (A9x23, (23, 29, 16), (4, 2))}
    for folds in FOLDS:
        arr, n, pitch = d_geo[folds]
        tag = folds or "none"
        cs[f"2d-nt1-{tag}"] = _case("2d", arr, pitch, n, folds, nt=1, foci=("generic", NF1[folds]), out="pic", apod=1)
        cs[f"2d-nt2-{tag}-clamp"] = _case("2d", arr, pitch, n, folds, clamp=True, nt=2, foci=("generic", NF2[folds]), out="pic", apod=2)
        cs[f"2d-nt4-{tag}-pin"] = _case("2d", A8x16, P3, (25, 28, 9) if folds in ("xy", "x") else (24, 27, 8), folds, clamp=(folds in ("x", "")), nt=4, foci=("generic", NF4[folds]),
                                        out="pic" if folds == "xy" else "p", pin="lattice2d")
    cs["2d-nt1-xy-clamp"] = _case("2d", A12x16, P3, (60, 40, 9), "xy", clamp=True, nt=1, foci=("generic", 1), out="pic")
    cs["2d-nt2-xy"] = _case("2d", A8x16, (3, 2), (25, 28, 23), "xy", nt=2, foci=("wheel", 6), out="pic", h=(1.0, 1.25, 0.8))
    cs["2d-nt1-xy-pitch1"] = _case("2d", A16, (1, 2), (25, 29, 9), "xy", nt=1, foci=("generic", 1), out="pic")
    cs["2d-nt1-xy-pin-noncomplex"] = _case("2d", A8x16, P3, (25, 28, 8), "xy", nt=1, foci=("generic", 2), out="pi", pin="lattice2d", apod=1)
    # ---- kernel 2f: one steering vector in the launch.  NM = 1 / 2 / 3 x {fp16, e4m3} x clamp; DIR; the fold patterns
    for arith in ("fp16", "e4m3"):
        f8 = arith == "e4m3"
        cs[f"2f-nm1-{arith}"] = _case("2f", A16, P3, (36, 40, 32), "xy", e4m3=f8, fp16=not f8, foci=("axis", 1), frag=("1 row tile(s)",))
        cs[f"2f-nm2-{arith}"] = _case("2f", A16, P3, (60, 40, 32), "xy", e4m3=f8, fp16=not f8, foci=("axis", 1), frag=("2 row tile(s)",), out="pi")
        cs[f"2f-nm3-{arith}"] = _case("2f", A18x16, (6, 6), (200, 40, 120), "xy", e4m3=f8, fp16=not f8, foci=("axis", 1), frag=("3 row tile(s)",), h=(0.5, 0.5, 0.5))
    cs["2f-nm1-clamp"] = _case("2f", A8x16, P3, (36, 40, 17), "xy", clamp=True, foci=("axis", 1), frag=("1 row tile(s)",), out="pi")
    cs["2f-nm2-clamp"] = _case("2f", A12x16, P3, (60, 40, 17), "xy", clamp=True, foci=("axis", 1), frag=("2 row tile(s)",))
    cs["2f-nm3-clamp"] = _case("2f", A18x16, (6, 6), (200, 40, 120), "xy", clamp=True, foci=("axis", 1), frag=("3 row tile(s)",), h=(0.5, 0.5, 0.5), z0=-2.0)
    cs["2f-nm1-clamp-e4m3-dev"] = _case("2f", A16, P3, (36, 40, 16), "xy", clamp=True, e4m3=True, foci=("axis", 1), dev=True, z0=0.75, frag=("1 row tile(s)",))
    cs["2f-nm2-clamp-e4m3-dev"] = _case("2f", A16, P3, (60, 40, 16), "xy", clamp=True, e4m3=True, foci=("axis", 1), dev=True, z0=0.75, frag=("2 row tile(s)",))
    cs["2f-nm3-clamp-e4m3-dev"] = _case("2f", A18x16, (6, 6), (200, 40, 120), "xy", clamp=True, e4m3=True, foci=("axis", 1), dev=True, h=(0.5, 0.5, 0.5), z0=0.375, frag=("3 row tile(s)",))
    cs["2f-dir-piston"] = _case("2f", A18x16, (6, 6), (200, 40, 32), "xy", foci=("axis", 1), dirv=True, h=(0.5, 0.5, 0.5), frag=("1 row tile(s)", "piston directivity in the tables"))
    cs["2f-dir-both-clamp"] = _case("2f", A8x16, P3, (36, 40, 17), "xy", clamp=True, foci=("axis", 1), dirv=True, absorb=ABSORB, apod=1,
                                    frag=("1 row tile(s)", "piston directivity in the tables", "uniform absorption in the tables"))
    cs["2f-y-xslab"] = _case("2f", A16, P3, (60, 40, 23), "xy", slab=(7, 40), foci=("axis", 1), frag=("2 row tile(s)",), apod=1)      # an x-slab of a centred grid keeps the y fold only
    cs["2f-none-shifted"] = _case("2f", A9x23, (4, 2), (31, 45, 16), "", foci=("generic", 1), apod=2, frag=("1 columns for 1 foci x 1 images",))
    cs["2f-x-yaxis-focus"] = _case("2f", A20x12, P3, (30, 50, 20), "x", foci=("yaxis", 1), apod=1, out="pi")
    cs["2f-xy-odd-aniso"] = _case("2f", A8x16, (3, 2), (37, 41, 23), "xy", foci=("axis", 1), h=(1.0, 0.8, 1.25), apod=2)      # odd nx and ny under both folds, three distinct spacings
    cs["2f-xy-pitch1"] = _case("2f", A16, (1, 2), (31, 41, 16), "xy", e4m3=True, foci=("axis", 1), out="pi")      # (voxels on both symmetry planes: the e4m3 rule's raised constant)
    # (320 uniformly driven elements focused 12 mm deep: the focal peak is large enough for the e4m3 rule to admit a grid through the element plane)
    cs["2f-y-xaxis-focus-clamp"] = _case("2f", A16x20, (3, 2), (36, 40, 17), "y", clamp=True, e4m3=True, foci=("xaxis", 1), frag=("2 row tile(s)",))
    # ---- planner exits: the kernel that takes over
    cs["exit-poor-coset-fill-2d"] = _case("2d", A8x16, (6, 6), (26, 24, 16), "xy", nt=1, foci=("generic", 1), out="pi")             # coset_fill 0.27 < 0.6, not complex
    cs["exit-nt4-complex-2c"] = _case("2c", A8x16, P3, (25, 28, 9), "xy", nt=4, foci=("generic", 5), out="pic")
    cs["exit-nt4-poor-fill-2c"] = _case("2c", A8x16, (6, 6), (26, 24, 16), "xy", nt=4, foci=("generic", 5))
    cs["exit-row-tile-fill-2c"] = _case("2c", A8x16, (6, 6), (22, 24, 16), "xy", nt=1, foci=("generic", 1))                         # 11 computed voxels per 24-voxel row tile
    cs["exit-fractional-pitch-2c"] = _case("2c", A8x16, (2.5, 2.5), (25, 28, 16), "xy", nt=1, foci=("generic", 1), out="pic")
    cs["exit-padding-doubles-2c"] = _case("2c", (9, 9), P3, (25, 28, 16), "xy", nt=1, foci=("generic", 2))                          # 81 elements in 256 K slots
    cs["exit-rolled-element-dir"] = _case("dir", A8x16, P3, (25, 28, 16), "xy", foci=("generic", 1), dirv=True, rolled=True, frag=("(piston directivity)",))
    return cs


ALL_CASES = _build_cases()
CASES = {k: c for k, c in ALL_CASES.items() if not c["dev"]}
DEV_CASES = {k: c for k, c in ALL_CASES.items() if c["dev"]}      # need OLX_FP8_CORRECTION=1, which only a developer build honours (module docstring)
BIG = [k for k in ALL_CASES if k.startswith("2f-nm3-")]
EPILOGUE_SETS = [f"{k}-epi-{{}}-nz{nz}" for k in ("2g", "2e") for nz in (32, 23)]


# ---- the planner's decision for lattice arrays, restated (decide_variant in olx_plan.cpp, olx_field_plan in olx.hip) ----------------------------------
def tile_fill(width, m):
    blk = 4 * m
    return width / (-(-width // blk) * blk)


def plan_rule(case, report=None):
    """The variant string up to '>' plus the fragments that follow it, from the generators alone.  `report`, a dict, receives the intermediate
    quantities the coverage test reads (columns per tile, NM, fills, positions of a coset)."""
    q = planq()
    pos, ori, size, xs, ys, zs = geometry(case)
    n = len(pos)
    h = np.array([xs[1] - xs[0], ys[1] - ys[0], zs[1] - zs[0]])
    nx, ny, nz = case["n"]
    xb, xc = case["slab"] or (0, nx)
    delays, ap = steering(case)
    F = len(delays)
    area = size[:, 0] * size[:, 1] * 1e-6
    outs = OUTPUTS[case["out"]]
    cplx = "complex" in outs
    modifier = case["dirv"] or case["absorb"] > 0
    pin = case["pin"]
    assert pin in (None, "lattice", "lattice2d")
    force4 = pin is not None
    rep = report if report is not None else {}
    # olx_field_plan: clamp over the real elements, lattice detection (real code: bounds over real AND virtual lattice points), the mirror folds
    lo = np.array([xs[xb], ys[0], zs[0]]); hi = np.array([xs[xb + xc - 1], ys[-1], zs[-1]])
    dmin = 0.5 * h.min()
    cls = distance_class(pos, xs[xb:xb + xc], ys, zs)
    info = np.zeros(8, dtype=np.int32)
    soa, soa_p = _d(pos.T * 1e-3)
    _, hp = _d(h); _, lop = _d(lo); _, hip_ = _d(hi)
    q.olq_lattice(n, soa_p, hp, lop, hip_, ctypes.c_double(dmin), info.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    lat_ok_geo, ax, ay, lmx, lmy, nsa, nsb, lat_clamp = (int(v) for v in info)
    rep.update(lattice=bool(lat_ok_geo), nsa=nsa, nsb=nsb)
    dir_lattice = bool(modifier and not cplx and (not case["dirv"] or not ori.any()))
    allow_shared = (not modifier) or dir_lattice

    def mirror(axis, coords):       # the element set symmetric about the grid's centre plane of this axis (olx_field_plan's mirror_perm, 1e-12 m)
        ctr = 0.5 * (coords[0] + coords[-1])
        img = pos * 1e-3
        img = img.copy(); img[:, axis] = 2 * ctr - img[:, axis]
        d = np.abs(img[:, None, :] - pos[None, :, :] * 1e-3).max(axis=2)
        perm = d.argmin(axis=1)
        return perm.astype(np.int32) if (d[np.arange(n), perm] <= 1e-12).all() and len(set(perm)) == n else None
    perm_x = mirror(0, xs) if (allow_shared and xb == 0 and xc == nx) else None
    perm_y = mirror(1, ys) if allow_shared else None
    mx, my = (2 if perm_x is not None else 1), (2 if perm_y is not None else 1)
    wx, wy = xc - (xc // 2 if mx == 2 else 0), ny - (ny // 2 if my == 2 else 0)
    lat_ok = bool(allow_shared and lat_ok_geo and tile_fill(wx, lmx) >= 0.5 and tile_fill(wy, lmy) >= 0.5)
    cl_plain = "clamp" if cls == "clamp" else "noclamp"
    dir_tail = ["(" + ", ".join((["piston directivity"] if case["dirv"] else []) + (["uniform absorption"] if case["absorb"] > 0 else [])) + ")"]
    if modifier and not (lat_ok and dir_lattice):
        return f"field_accum_dir_k<4,{cl_plain}>", dir_tail

    def coset_fill(nt):
        t16 = q.olq_coset_tiles16(wx, wy, lmx, lmy, nt)
        return 2.0 * wx * wy / (16.0 * t16) if t16 > 0 else 0.0

    ident = np.arange(n, dtype=np.int32)
    (pxa, pxp), (pya, pyp) = _i(perm_x if perm_x is not None else ident), _i(perm_y if perm_y is not None else ident)
    (_, dp), (_, app), (_, arp) = _d(delays), _d(ap), _d(area)

    def pack(maxc):
        sizes = np.zeros(64, dtype=np.int32); mt = ctypes.c_int(0)
        nt_ = q.olq_pack(n, F, int(mx == 2), int(my == 2), pxp, pyp, dp, app, arp, ctypes.c_double(F0), maxc, sizes.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), 64, ctypes.byref(mt))
        return [int(v) for v in sizes[:nt_]], mt.value
    tiles, max_tgt = pack(32)
    # (kernels 2a / 2b: a launch whose steering is symmetric under every fold and holds one focus -- no such row in this table)
    assert lat_ok or sum(tiles) >= 2, "a row for kernel 2a / 2b: not this table's business"
    # the e4m3 rule (real code); the developer pin forces it
    cut = -1
    if lat_ok and not (case["fp16"] or cplx or modifier):
        (_, fp), (_, op) = _d(foci_of(case)), _d([xs[0], ys[0], zs[0]])
        _, gnp = _i([nx, ny, nz])
        cut = q.olq_fp8_first_plane(n, soa_p, arp, app, F, fp, op, hp, gnp, xb, xc)
    if case["dev"]:
        cut = 0 if (lat_ok and not modifier) else -1
    if cut > 0 and not q.olq_fp8_split_pays(xc, ny, nz, F, cut):
        cut = -1
    assert cut <= 0, "a split launch: left out of this matrix"
    fp8_want = cut == 0
    use_lattice = lat_ok
    wide = len(tiles) == 1 and tiles[0] > 16
    if (len(tiles) > 1 or (wide and fp8_want)) and use_lattice and not cplx and pin is None and coset_fill(2) >= 0.6:
        tiles, max_tgt = pack(16)
    nt = 1
    for t in tiles:
        while nt * 8 < t:
            nt *= 2
    rep.update(tiles=tiles, nt=nt, max_targets=max_tgt, fills={k: coset_fill(k) for k in (1, 2, 4)} if lat_ok_geo else {}, wx=wx, wy=wy, pitch=(lmx, lmy))
    if use_lattice and nt >= 4 and not force4 and (cplx or coset_fill(nt) < 0.6):
        use_lattice = False
    counts = f"{sum(tiles)} columns for {F} foci x {mx * my} images in {len(tiles)} tile(s)"
    if not use_lattice:
        if modifier:
            return f"field_accum_dir_k<4,{cl_plain}>", dir_tail
        return f"field_mfma_k<mt{4 if nz >= 48 else 1},nt{nt},mx{mx},my{my},flat,{cls}>", [counts]
    use_coset = not cplx and pin != "lattice2d"
    if 0 < coset_fill(nt) < 0.6 and pin != "lattice":
        use_coset = False
    use_toep = use_coset and sum(tiles) == 1 and pin != "lattice"
    use_cosetp = use_coset and not use_toep and nt == 2 and pin != "lattice"
    cl = "clamp" if (cls == "clamp" or lat_clamp) else "noclamp"
    f8 = ",fp8corr" if (fp8_want and use_coset and nt <= 2 and not modifier) else ""
    tail = [counts]
    if not use_coset:
        if modifier:
            return f"field_accum_dir_k<4,{cl_plain}>", dir_tail
        name = f"field_lattice_k<mt4,nt{nt},mx{mx},my{my},flat,{cl}>"
    elif use_toep:
        kyw = ctypes.c_int(0)
        nm = q.olq_toep_nm(ax, lmx, lmy, 1, wx, wy, nz, int(dir_lattice), ctypes.byref(kyw))
        rep.update(nm=nm, kxa=(wx - 1) // lmx + 1)
        name = f"field_toep_k<mx{mx},my{my},flat,{cl}{f8}>"
        tail.append(f"{nm} row tile(s) x {kyw.value} y positions per block")
    else:
        name = f"field_coset{'p' if use_cosetp else ''}_k<nt{nt},mx{mx},my{my},flat,{cl}{f8}>"
        rep.update(kx=(wx - 1) // (2 * lmx) + 1, ky=(wy - 1) // lmy + 1)
    if case["dirv"]:
        tail.append("+piston directivity in the tables")
    if case["absorb"] > 0:
        tail.append("+uniform absorption in the tables")
    return name, tail


def real_variant(case):
    """The whole string of the REAL decision (olxplan::decide_variant, through tools/plan_query.cpp) for the plan run_lcase makes of the case: the same
    elements, steering, grid, slab, outputs, flags and pins; the foci are known where kernel 1 makes the steering, inferred from the delays otherwise.
    Developer rows ask the library built with -DOLX_DEV_PINS."""
    pos, ori, size, xs, ys, zs = geometry(case)
    delays, ap = steering(case)
    return real_variant_of(pos * 1e-3, size[:, 0] * size[:, 1] * 1e-6, delays, ap, xs, ys, zs, F0, C, RHO, P0, OUTPUTS[case["out"]],
                           foci=foci_of(case) if _solve(case) else None, slab=case["slab"], fp16=case["fp16"], directivity=case["dirv"], aligned=not ori.any(),
                           size=size[0] * 1e-3, absorb=case["absorb"], stored=case["stored"], pin=case["pin"], fp8_pin="1" if case["dev"] else None, dev=case["dev"])


def _agrees(case, label):
    """plan_rule, the independent restatement, against the real decision: the same string up to '>' and every later fragment it predicts."""
    line = real_variant(case)
    name, tail = plan_rule(case)
    assert line.split(">")[0] + ">" == name, (label, line, name)
    for frag in tail:
        assert frag in line, (label, frag, line)
    return line


# ---- CPU tests -------------------------------------------------------------------------------------------------------------------------------------
def test_every_row_reaches_its_variant_in_the_real_decision():
    """Without a GPU: decide_variant itself produces, for every row of the table (developer rows included), the string the GPU tests wait for -- `want` up
    to '>' and every entry of `frag` after it -- and plan_rule agrees with it on every row, on the slab sets and on the seeded sweep's draws."""
    for cid, case in ALL_CASES.items():
        line = _agrees(case, cid)
        assert line.split(">")[0] + ">" == case["want"], (cid, line, case["want"])
        for frag in case["frag"]:
            assert frag in line, (cid, frag, line)
        assert "from plane" not in line, (cid, line)
    for which in SLAB_SETS:
        case, want_whole, want_part = _slab_case(which)
        assert real_variant(case).startswith(want_whole), (which, real_variant(case))
        for slab in ((0, 10), (10, 17), (27, 9)):
            assert _agrees(dict(case, slab=slab), (which, slab)).startswith(want_part), (which, slab)
    for q, case in enumerate(_sweep_cases()):
        _agrees(case, f"sweep-{q}")


def _kernel(c):
    return c["want"].split("<")[0]


def test_case_table_covers_every_instantiation():
    allc = list(ALL_CASES.values())
    want = [c["want"] for c in allc]
    prod = [c["want"] for c in CASES.values()]
    assert len(CASES) >= 90, len(CASES)
    folds = [(mx, my) for mx, my in FOLDS.values()]
    # kernel 2d: NT = 1 / 2 through complex output, NT = 4 under the lattice2d pin, every fold pattern, both clamp values
    for nt in (1, 2, 4):
        for mx, my in folds:
            hits = [c for c in CASES.values() if c["want"].startswith(f"field_lattice_k<mt4,nt{nt},mx{mx},my{my},")]
            assert any(("complex" in OUTPUTS[c["out"]] and c["pin"] is None) if nt < 4 else c["pin"] == "lattice2d" for c in hits), (nt, mx, my)
            assert nt < 4 or all(c["pin"] == "lattice2d" for c in hits), (nt, mx, my)          # (the planner leaves the family at NT = 4 otherwise)
        for cl in ("clamp", "noclamp"):
            assert any(w.startswith(f"field_lattice_k<mt4,nt{nt},") and w.endswith(f",{cl}>") for w in prod), (nt, cl)
    # kernel 2e: every fold pattern and both clamp values per NT; NT = 2 and the single column only under the pin; e4m3 for NT = 1 / 2; DIR three ways
    for nt in (1, 2, 4):
        for mx, my in folds:
            assert any(w.startswith(f"field_coset_k<nt{nt},mx{mx},my{my},") for w in prod), (nt, mx, my)
        for cl in ("clamp", "noclamp"):
            assert any(w.startswith(f"field_coset_k<nt{nt},") and f",{cl}" in w for w in prod), (nt, cl)
        if nt <= 2:
            assert any(w.startswith(f"field_coset_k<nt{nt},") and w.endswith(",noclamp,fp8corr>") for w in prod), nt
            assert any(w.startswith(f"field_coset_k<nt{nt},") and w.endswith(",clamp,fp8corr>") for w in (c["want"] for c in DEV_CASES.values())), nt
    assert all(c["pin"] == "lattice" for c in allc if c["want"].startswith("field_coset_k<nt2"))
    assert any(c["pin"] == "lattice" and "1 columns for 1 foci x 4 images" in c["frag"] for c in allc if _kernel(c) == "field_coset_k")
    for kern in ("field_coset_k", "field_cosetp_k"):
        mods = {(c["dirv"], c["absorb"] > 0) for c in CASES.values() if _kernel(c) == kern}
        assert mods >= {(True, False), (False, True), (True, True), (False, False)}, (kern, mods)
    # kernel 2g: folds 4 x clamp 2 x {fp16, e4m3 corrections} (clamp with e4m3 on the developer list), DIR under >= 2 fold patterns and both clamp values
    for mx, my in folds:
        for cl in ("clamp", "noclamp"):
            for f8 in ("", ",fp8corr"):
                pool = want if (cl == "clamp" and f8) else prod
                assert f"field_cosetp_k<nt2,mx{mx},my{my},flat,{cl}{f8}>" in pool, (mx, my, cl, f8)
    gdir = [c for c in CASES.values() if _kernel(c) == "field_cosetp_k" and (c["dirv"] or c["absorb"] > 0)]
    assert len({c["folds"] for c in gdir}) >= 2 and {",clamp" in c["want"] for c in gdir} == {True, False}
    # the three epilogues of 2g (and 2e), with nz % 4 == 0 and ragged
    for kern in ("field_cosetp_k", "field_coset_k"):
        for ragged in (False, True):
            epi = {(c["out"], c["stored"]) for c in CASES.values() if _kernel(c) == kern and (c["n"][2] % 4 != 0) == ragged}
            assert epi >= {("p", False), ("pi", True), ("i", True)}, (kern, ragged, epi)
    # kernel 2f: NM = 1 / 2 / 3 x {fp16, e4m3} x clamp, DIR (NM = 1), the four fold patterns
    for nm in (1, 2, 3):
        for cl in ("clamp", "noclamp"):
            for f8 in ("", ",fp8corr"):
                pool = ALL_CASES if (cl == "clamp" and f8) else CASES
                assert any(c["want"].startswith("field_toep_k<") and c["want"].endswith(f",{cl}{f8}>") and f"{nm} row tile(s)" in c["frag"] for c in pool.values()), (nm, cl, f8)
    assert any(_kernel(c) == "field_toep_k" and c["dirv"] and "1 row tile(s)" in c["frag"] for c in CASES.values())
    for mx, my in folds:
        assert any(w.startswith(f"field_toep_k<mx{mx},my{my},") for w in prod), (mx, my)
    assert any(_kernel(c) == "field_toep_k" and c["slab"] for c in CASES.values())
    # planner exits
    exits = {k: c["want"].split("<")[0] for k, c in CASES.items() if k.startswith("exit-")}
    assert sorted(exits.values()) == sorted(["field_lattice_k", "field_mfma_k", "field_mfma_k", "field_mfma_k", "field_mfma_k", "field_mfma_k", "field_accum_dir_k"]), exits
    # e4m3 only where the table says so, never with modifiers, complex output or the opt-out flag
    for k, c in ALL_CASES.items():
        assert ("fp8corr" in c["want"]) == c["e4m3"], k
        assert not (c["e4m3"] and (c["fp16"] or c["dirv"] or c["absorb"] or "complex" in OUTPUTS[c["out"]])), k
    # shape edges, per kernel they apply to
    by = {kern: [c for c in CASES.values() if _kernel(c) == kern] for kern in ("field_lattice_k", "field_coset_k", "field_cosetp_k", "field_toep_k")}
    for kern, cs in by.items():
        arrs = {c["arr"] for c in cs}
        assert arrs & {A20x12, A9x23}, (kern, "padded super-blocks")
        assert A16x20 in arrs, (kern, "odd number of super-block rows")
        assert len({c["pitch"][0] != c["pitch"][1] for c in cs}) == 2, (kern, "unequal pitches")
        assert any(len(set(c["h"])) == 3 for c in cs), (kern, "anisotropic spacing")
        # odd and even nx / ny AGAINST each fold: with an odd count the centre row is its own mirror image (an x-slab folds y only)
        assert {c["n"][0] % 2 for c in cs if "mx2" in c["want"]} == {0, 1} and {c["n"][1] % 2 for c in cs if "my2" in c["want"]} == {0, 1}, (kern, "odd and even nx / ny under a fold")
        pitches = {p for c in cs for p in c["pitch"]}
        assert pitches >= {1, 2, 3} and pitches & {4, 5, 6}, (kern, pitches)
        assert {a[0] for a in (c["apod"] for c in cs)} == {"uniform", "maxangle", "piecewise"}, (kern, "apodization")
    assert {c["arr"] for c in by["field_cosetp_k"]} >= {A8x16, A16, A20x16, A16x32}                    # nsa = 1 / 2 / 3, nsbp = 4
    for kern in ("field_coset_k", "field_cosetp_k", "field_toep_k"):
        nzs = {c["n"][2] for c in by[kern]}
        assert nzs & {16, 32} and nzs & {17, 23, 37}, (kern, nzs)
    assert {16, 32, 17, 23, 37} <= {c["n"][2] for c in CASES.values()}
    assert {c["n"][2] for c in by["field_lattice_k"]} >= {8, 9}
    assert any(c["z0"] == c["h"][2] for c in CASES.values())                                           # a grid one voxel above the element plane
    assert any(c["foci"][0] == "wheel" for c in by["field_cosetp_k"]) and any(c["foci"][0] == "wheel" for c in by["field_lattice_k"])
    assert any("in 3 tile(s)" in f for c in by["field_cosetp_k"] for f in c["frag"]) and any("in 2 tile(s)" in f and c["e4m3"] for c in by["field_cosetp_k"] for f in c["frag"])
    # largest KX x KY block of the NT = 2 shape at pitch 3 (the table-reuse test's restatement of the partition)
    shapes = block_shapes(G_BASE, (True, True))
    assert (3, 11) in shapes and max(kx * ky for kx, ky in shapes) == 33
    for kern, nt in (("field_cosetp_k", 2), ("field_coset_k", 2)):      # ... and cases of 2g and of 2e's NT = 2 form run exactly that partition: pitch 3, G_BASE, both folds
        assert any(c["n"] == G_BASE and c["pitch"] == P3 and c["want"].startswith(f"{kern}<nt{nt},mx2,my2,") for c in by[kern]), kern
    # size caps
    for k, c in ALL_CASES.items():
        assert n_terms(c) <= (CAP_BIG if k in BIG else CAP), (k, n_terms(c))
    assert len(BIG) <= MAX_BIG


def test_generators_and_table_follow_the_planning_rule():
    seen_cols, seen_tgt, kx_nt, ky_max = set(), 0, {1: 0, 2: 0, 4: 0}, 0
    for cid, case in ALL_CASES.items():
        rep = {}
        name, tail = plan_rule(case, rep)
        assert name == case["want"], (cid, name, case["want"])
        line = name + " " + "; ".join(tail)
        for frag in case["frag"]:
            assert frag in line, (cid, frag, line)
        if "tiles" in rep:
            seen_cols.update(rep["tiles"]); seen_tgt = max(seen_tgt, rep["max_targets"])
        if "kx" in rep:
            kx_nt[rep["nt"]] = max(kx_nt[rep["nt"]], rep["kx"]); ky_max = max(ky_max, rep["ky"])
            assert min(rep["fills"][rep["nt"]], 1.0) >= 0.6, (cid, rep["fills"])
        if cid.startswith("2g-") and "nsa" in cid:
            assert (rep["nsa"], (rep["nsb"] + 1) & ~1) == {"2g-nsa1-8x16": (1, 2), "2g-nsa3-20x16": (3, 2), "2g-nsbp4-16x32": (2, 4)}[cid], (cid, rep)
    assert seen_cols >= {1, 2, 8, 9, 16, 17, 32}, sorted(seen_cols)             # column counts at the NT boundaries
    silent = [cid for cid, c in CASES.items() if c["apod"][0] != "uniform" and (steering(c)[1] == 0).any()]
    assert len(silent) >= 10, silent                                             # zero weights occur (angle-limited drives)
    assert seen_tgt == 4                                                         # on-axis foci: 3 - 4 store targets per column
    assert kx_nt[1] > 6 and kx_nt[2] > 3 and kx_nt[4] > 2 and ky_max > 11, (kx_nt, ky_max)      # position grids cut into unequal parts
    # a grid through the element plane with voxels ON real and ON virtual lattice points
    for cid in ("2g-xy-clamp", "2e-nt1-x-clamp", "2d-nt1-xy-clamp", "2f-nm2-clamp"):      # one clamp case per kernel
        c = ALL_CASES[cid]
        pos, _, _, xs, ys, zs = geometry(c)
        (nax, nay), (px, py) = c["arr"], (c["pitch"][0] * c["h"][0] * 1e-3, c["pitch"][1] * c["h"][1] * 1e-3)
        a, b = np.meshgrid(np.arange(8 * -(-nax // 8)), np.arange(16 * -(-nay // 16)), indexing="ij")      # the padded lattice: 8 x 8 super-blocks, rows in pairs
        lx, ly, real = (a - (nax - 1) / 2) * px, (b - (nay - 1) / 2) * py, (a < nax) & (b < nay)
        hit = np.isclose(xs[:, None, None], lx[None]).any(axis=0) & np.isclose(ys[:, None, None], ly[None]).any(axis=0)      # lattice points that carry a voxel column
        assert np.isclose(zs, 0).any() and (hit & real).any() and (hit & ~real).any(), cid
    # the seeded sweep's draws spread over the kernels
    names = {_sweep_name(plan_rule(c)[0]) for c in _sweep_cases()}
    assert len(names) >= 4, names
    assert all(n_terms(c) <= CAP for c in _sweep_cases())


@functools.lru_cache(maxsize=None)
def reference0(cid, wrong=None):
    """Oracle volume of focus 0 over the whole grid.  wrong = "row": the last element row silent; "shift": the array displaced by one pitch along x."""
    case = ALL_CASES[cid]
    pos, ori, size, xs, ys, zs = geometry(case)
    delays, ap = steering(case)
    d, a = delays[0], ap[0].copy()
    pos_m = pos * 1e-3
    dirv, absorb = modifiers(case)
    if wrong == "row":
        a[np.arange(len(a)) % case["arr"][1] == case["arr"][1] - 1] = 0.0
    if wrong == "shift":
        pos_m = pos_m + [case["pitch"][0] * case["h"][0] * 1e-3, 0.0, 0.0]
    ref = co.field_on_grid(xs, ys, zs, pos_m, size[:, 0] * size[:, 1] * 1e-6, d, a, F0, C, P0, dmin=0.5 * min(xs[1] - xs[0], ys[1] - ys[0], zs[1] - zs[0]),
                           directivity=dirv, absorption=absorb)
    ref.setflags(write=False)
    return ref


def _distance(case, a, b):
    """Per requested output: max |a - b| over the planned volume in units of that output's reference maximum."""
    xb, xc = case["slab"] or (0, case["n"][0])
    a, b = a[xb:xb + xc], b[xb:xb + xc]
    mx = np.abs(b).max()
    ia, ib = fo.intensity_wcm2(np.abs(a), RHO, C), fo.intensity_wcm2(np.abs(b), RHO, C)
    return {"pmag": np.abs(np.abs(a) - np.abs(b)).max() / mx, "complex": np.abs(a - b).max() / mx, "intensity": np.abs(ia - ib).max() / ib.max()}


@pytest.mark.parametrize("cid", list(ALL_CASES))
def test_oracle_alone_and_sensitivity(cid):
    """The reference is finite with a positive maximum, and the errors the matrix is for are visible in it: a silent last element row (a padding-slot
    error), the array displaced by one pitch along x (a coset / Toeplitz offset error) and, where a fold has distinct images of focus 0, the mirror
    image stored in its place (a store-target error) each move the reference by more than ten gates of every output compared.  (A focus ON a fold's
    plane has one steering vector for both images of that fold: a swapped store target writes the same numbers -- kernel 2f's folded cases.)"""
    case = ALL_CASES[cid]
    ref = reference0(cid)
    assert np.isfinite(ref.view(np.float64)).all() and np.abs(ref).max() > 0
    wrongs = {"row": reference0(cid, "row"), "shift": reference0(cid, "shift")}
    f0 = foci_of(case)[0]
    mx, my = (int(v) for v in re.search(r"mx(\d),my(\d)", case["want"]).groups()) if "mx" in case["want"] else (1, 1)
    if mx == 2 and abs(f0[0]) > 1e-9:
        wrongs["mirror-x"] = ref[::-1]
    if my == 2 and abs(f0[1]) > 1e-9:
        wrongs["mirror-y"] = ref[:, ::-1]
    if (mx == 2 or my == 2) and _kernel(case) != "field_toep_k" and "1 columns for 1 foci x 4 images" not in case["frag"]:
        assert any(k.startswith("mirror") for k in wrongs), cid
    for what, w in wrongs.items():
        dist = _distance(case, w, ref)
        for o in OUTPUTS[case["out"]]:
            assert dist[o] > 10 * GATES[o], (cid, what, o, dist[o])


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------------------
ENV = ("OLX_FIELD_VARIANT", "OLX_INTENSITY_STORED", "OLX_FP8_CORRECTION")


def _solve(case):
    """Steering by kernel 1 on the device (the library then knows the foci), except for the piecewise-linear apodization: the device's weights agree
    with the oracle's to 1e-12 (tests/test_gpu_bf.py), not to the bit setup_ctx asks for, so those cases hand the oracle's table in (olx_set_steering, the
    run_simulation seam).  No e4m3 case is among them: an angle-limited drive does not reach the N_eff the rule asks for."""
    return case["apod"][0] != "piecewise"


def run_lcase(ctx, case, label, monkeypatch, want=True):
    """Environment, elements, steering and per-term factors of a case, then test_gpu_field_matrix.measure; a variant that says fp8corr also keeps the
    stated e4m3 bound.  Returns (variant, worst error per output, volumes [focus][output])."""
    for k, v in zip(ENV, (case["pin"], "1" if case["stored"] else None, "1" if case["dev"] else None)):
        monkeypatch.setenv(k, v) if v else monkeypatch.delenv(k, raising=False)
    pos, ori, size, xs, ys, zs = geometry(case)
    pos_m, area, d, ap = setup_ctx(ctx, pos, ori, size, foci_of(case), apod=case["apod"], solve=_solve(case))
    dirv, absorb = modifiers(case)
    if dirv is not None:
        ctx.set_element_apertures(dirv[0], dirv[2])
    ctx.field_absorption(absorb)
    outputs = OUTPUTS[case["out"]]
    flags = (nat.FIELD_FP16_CORRECTION if case["fp16"] else 0) | (nat.FIELD_DIRECTIVITY if dirv is not None else 0)
    try:        # test_gpu_field_matrix.measure: plan, the variant asserted before anything is compared, launch, every output of every focus against the oracle at the gates
        name, worst, vols, _ = measure(ctx, xs, ys, zs, pos_m, area, d, ap, outputs, want_variant=case["want"] if want else None, slab=case["slab"], label=label,
                                       extra_flags=flags, fragments=case["frag"] if want else (), directivity=dirv, absorption=absorb, tag="LMATRIX")
    finally:
        ctx.field_absorption(0.0)
    assert "from plane" not in name, (label, name)          # split launches are not this matrix's
    if want and _kernel(case) in ("field_coset_k", "field_cosetp_k", "field_toep_k", "field_lattice_k"):
        assert ("fp8corr" in name) == case["e4m3"], (label, name)
    if "fp8corr" in name and not case["dev"] and "pmag" in outputs:       # what a plan that names fp8corr promises (include/olx.h); the developer pin bypasses the rule that makes the promise
        assert worst["pmag"] <= FP8_BOUND, (label, name, worst)
    return name, worst, vols


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(CASES))
def test_lattice_matrix_case_matches_oracle(ctx, cid, monkeypatch):
    run_lcase(ctx, CASES[cid], cid, monkeypatch)


@pytest.mark.gpu
@pytest.mark.skipif(not DEV_LIB, reason="OLX_FP8_CORRECTION=1 is honoured by developer builds only (runs in the debug-library child of test_gpu_debug_bounds.py)")
@pytest.mark.parametrize("cid", list(DEV_CASES))
def test_lattice_matrix_dev_pin_case_matches_oracle(ctx, cid, monkeypatch):
    run_lcase(ctx, DEV_CASES[cid], cid, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", EPILOGUE_SETS)
def test_one_output_alone_has_the_bits_of_the_two_output_launch(ctx, pattern, monkeypatch):
    """|p| alone (the product's plan: its own epilogue) and intensity alone carry the bits of the launch that stores both (OLX_INTENSITY_STORED=1)."""
    both = run_lcase(ctx, CASES[pattern.format("pi-stored")], pattern.format("pi-stored") + " (bits)", monkeypatch)[2]
    p_only = run_lcase(ctx, CASES[pattern.format("p")], pattern.format("p") + " (bits)", monkeypatch)[2]
    i_only = run_lcase(ctx, CASES[pattern.format("i-stored")], pattern.format("i-stored") + " (bits)", monkeypatch)[2]
    for f in range(len(both)):
        assert np.array_equal(p_only[f]["pmag"], both[f]["pmag"]), (pattern, f)
        assert np.array_equal(i_only[f]["intensity"], both[f]["intensity"]), (pattern, f)


SLAB_SETS = {   # kernel of the slabs: foci, apodization, variant of the whole grid, variant of an x-slab (the x fold is lost: half the images)
    "2g": (("generic", 5), 1, "field_coset_k<nt4,mx2,my2,flat,noclamp>", "field_cosetp_k<nt2,mx1,my2,flat,noclamp>"),
    "2e-nt1": (("generic", 2), 2, "field_coset_k<nt1,mx2,my2,flat,noclamp>", "field_coset_k<nt1,mx1,my2,flat,noclamp>"),
    "2f": (("axis", 1), 1, "field_toep_k<mx2,my2,flat,noclamp>", "field_toep_k<mx1,my2,flat,noclamp>"),
}


def _slab_case(which):
    foci, apod, whole, part = SLAB_SETS[which]
    return _case("2g", A16, P3, (36, 40, 17), "xy", foci=foci, apod=apod, out="pi"), whole, part


@pytest.mark.gpu
@pytest.mark.parametrize("which", list(SLAB_SETS))
def test_x_slabs_keep_the_y_fold_and_tile_the_volume(ctx, which, monkeypatch):
    """The multi-GPU shard unit on a centred 16 x 16 array: three x-slabs of unequal width, each against the oracle; their concatenation against the
    whole-volume launch, which folds both axes -- another association of the same sums, so equal within the gate, not bit for bit."""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    case, want_whole, want_part = _slab_case(which)
    pos, ori, size, xs, ys, zs = geometry(case)
    pos_m, area, d, ap = setup_ctx(ctx, pos, ori, size, foci_of(case), apod=case["apod"], solve=_solve(case))
    ctx.field_absorption(0.0)
    outputs = OUTPUTS[case["out"]]
    _, _, whole, refs = measure(ctx, xs, ys, zs, pos_m, area, d, ap, outputs, want_variant=want_whole, label=f"lslabs-{which}-whole")
    parts = []
    for b, cnt in ((0, 10), (10, 17), (27, 9)):
        parts.append(measure(ctx, xs, ys, zs, pos_m, area, d, ap, outputs, want_variant=want_part, slab=(b, cnt), refs=refs, label=f"lslab-{which}-{b}+{cnt}")[2])
    for f in range(len(d)):
        mx = np.abs(refs[f]).max()
        imx = fo.intensity_wcm2(mx, RHO, C)
        for o, scale in (("pmag", mx), ("intensity", imx)):
            joined = np.concatenate([p[f][o] for p in parts], axis=0)
            assert joined.shape == whole[f][o].shape and np.abs(joined - whole[f][o]).max() / scale <= GATES[o], (which, f, o)


def test_slab_sets_follow_the_planning_rule():
    for which in SLAB_SETS:
        case, want_whole, want_part = _slab_case(which)
        assert plan_rule(case)[0] == want_whole, (which, plan_rule(case)[0])
        for slab in ((0, 10), (10, 17), (27, 9)):
            assert plan_rule(dict(case, slab=slab))[0] == want_part, (which, slab, plan_rule(dict(case, slab=slab))[0])


def _sweep_name(name):
    nt = re.search(r"nt(\d)", name)
    return name.split("<")[0] + (f"<nt{nt.group(1)}" if nt else "")


@functools.lru_cache(maxsize=None)
def _sweep_cases():
    rng = np.random.default_rng(SWEEP_SEED)
    arrays = [(A8x16, P3), (A8x16, (3, 2)), (A20x12, P3), (A16x20, (3, 2)), (A9x23, (4, 2)), (A12x16, (2, 3)), (A16, P3)]
    out = []
    for q in range(SWEEP_DRAWS):
        arr, pitch = arrays[rng.integers(len(arrays))]
        kind = str(rng.choice(["axis", "xaxis", "yaxis", "generic", "generic", "generic", "wheel"]))
        F = int(rng.choice([1, 2, 3, 5, 7])) if kind != "wheel" else int(rng.choice([4, 7]))
        F = 1 if kind == "axis" else F
        folds = str(rng.choice(["xy", "xy", "x", "y", ""]))
        n = (int(rng.choice([30, 33, 36])), int(rng.choice([40, 44, 45])), int(rng.choice([16, 17, 23, 32])))
        clamp = bool(rng.integers(2))
        c = _case("2g", arr, pitch, n, folds, clamp=clamp, foci=(kind, F), seed=int(rng.integers(1000)), out=str(rng.choice(["p", "pi", "pic", "i"])),
                  apod=0 if kind != "generic" else int(rng.integers(3)))
        c["want"] = None
        out.append(c)
    return tuple(out)


@pytest.mark.gpu
def test_seeded_sweep_over_the_default_planner(ctx, monkeypatch):
    """SWEEP_DRAWS random combinations of the table's axes, no pin, no expected variant: whatever the planner picks must pass the gates."""
    seen = []
    for q, case in enumerate(_sweep_cases()):
        seen.append(_sweep_name(run_lcase(ctx, case, f"sweep-{q}", monkeypatch, want=False)[0]))
    assert len(set(seen)) >= 4, seen
