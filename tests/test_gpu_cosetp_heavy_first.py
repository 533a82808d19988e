"""Kernel 2g (field_cosetp_k): the planner issues the position sets of a launch in the order of falling position count (olxplan::build_coset_blocks,
heavy_first; a stable sort of the coset order), the 16 plane blocks of a set still in a row on one XCD.  On the headline grid the 33-position blocks
come first and the 20-position blocks last.  Only the ORDER of the block records changes: which block computes which voxels, the arithmetic and the
kernel are the parent's, so the bits must not change -- with the order (the product), without it (OLX_EXP_CP_NOSORT=1 in developer builds: the A/B leg).

Cases (1 mm grid, 3 mm pitch; table, helpers and gates of tests/test_gpu_cosetp_fill_ahead.py and tests/test_gpu_cosetp_table_reuse.py, the names of
tests/test_gpu_cosetp_tile_addr.py): base_nz32 (33- and 30-position blocks: the order differs from the coset order), few_tiles_12x30 (one size:
the order is the coset order), ragged_nz23_e4m3, clamp_e4m3, fp16_corr, absorption_dir, no_mirror_fold, nsa3_20x16, nsbp4_16x32.

Every case: (a) the product's |p| volume of every focus against the fp64 C oracle at those files' gates, for ragged_nz23_e4m3 and clamp_e4m3 also the
debug library's launch with the e4m3 products forced; (b) an empty bounds report from the debug library; (c) in the debug library the bits with and
without OLX_EXP_CP_NOSORT=1 equal, and equal to the product's wherever both run the same products.  On the host: the real planner's records
(tools/plan_query.cpp: olq_blocks) are a permutation of the restated partition, never rise in position count along an XCD, and keep a set's plane
blocks 8 ids apart."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from openlifu_amd import _native as nat
from oracle import bf_oracle as bo, c_oracle as co

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plan_query as PQ                      # noqa: E402
import test_gpu_cosetp_fill_ahead as F       # noqa: E402  (case table, prepare / launch)
import test_gpu_cosetp_table_reuse as R      # noqa: E402  (block_shapes, the gates)

ROOT = R.ROOT
NAMES = ["base_nz32", "few_tiles_12x30", "ragged_nz23_e4m3", "clamp_e4m3", "fp16_corr", "absorption_dir", "no_mirror_fold", "nsa3_20x16", "nsbp4_16x32"]
FORCED = [c for c in NAMES if F.CASES[c].get("force")]
PIN = "OLX_EXP_CP_NOSORT"
COS_ZB = 16                                   # planes per block (olx_params.h)


def planner_records(name):
    """The block records of the real planner for a case (tools/plan_query.cpp, olq_blocks): ([records of the launch from the e4m3 cut on], [records of
    the launch below it]) of 8 ints {ibase, jbase, k0, npos, KY, ky_magic, KX, 0}."""
    cs = F.CASES[name]
    pos_m, area = F.elements_of(cs)
    foci = np.asarray(cs.get("foci", R.FOCI3))
    st = [bo.beamform(pos_m, np.zeros_like(pos_m), f, R.C) for f in foci]
    d, ap = np.array([s[0] for s in st]), np.array([s[1] for s in st])
    xs, ys, zs = F.coords_of(cs)
    flags = PQ.FLAG["pmag"] | (PQ.FLAG["fp16"] if cs.get("fp16") else 0)
    keep = [PQ._d(np.asarray(pos_m).T), PQ._d(area), PQ._d(d), PQ._d(ap), PQ._d(foci), PQ._d([xs[0], ys[0], zs[0]]), PQ._d([1e-3] * 3), PQ._i(list(cs["n"])),
            PQ._i([1, 0]), PQ._d([0.0, 0.0, cs.get("absorb", 0.0)])]
    (_, posp), (_, arp), (_, dp), (_, app), (_, fop), (_, op), (_, hp), (_, gnp), (_, mp), (_, ep) = keep
    cap = 1 << 16
    rec = np.zeros((cap, 8), dtype=np.int32)
    n_near, is_2g = ctypes.c_int(0), ctypes.c_int(0)
    cnt = PQ.planq().olq_blocks(len(pos_m), posp, arp, len(foci), dp, app, fop, op, hp, gnp, 0, cs["n"][0], ctypes.c_double(R.F0), ctypes.c_double(R.C),
                                ctypes.c_double(R.RHO), ctypes.c_double(R.P0), ctypes.c_uint(flags), mp, ep, None, None, None,
                                rec.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), cap, ctypes.byref(n_near), ctypes.byref(is_2g))
    assert 0 < cnt <= cap and is_2g.value == 1, (name, cnt, is_2g.value)
    rec = rec[:cnt]
    return rec[:cnt - n_near.value], rec[cnt - n_near.value:]


# ---- host tests (no GPU) ----
def test_the_planners_records_are_the_partition_heaviest_sets_first():
    reordered = 0
    for name in NAMES:
        cs = F.CASES[name]
        fold = cs.get("fold", True)
        shapes = [s for s in R.block_shapes(cs["n"], (fold, fold))]      # the coset order
        kblocks = -(-cs["n"][2] // COS_ZB)
        far, near = planner_records(name)
        rec = np.concatenate([far, near])
        # a permutation of the restated partition: one record per (position set, plane block), no (set, plane block) twice
        assert len(rec) == len(shapes) * kblocks, name
        live = rec[rec[:, 3] > 0]
        assert sorted(live[:, 3].tolist()) == sorted([a * b for a, b in shapes if a * b > 0] * kblocks), name
        assert (live[:, 3] == live[:, 6] * live[:, 4]).all() and (rec[:, 7] == 0).all()
        assert len({(int(r[0]), int(r[1]), int(r[2])) for r in live}) == len(live), name
        for side in (far, near):      # each side of the e4m3 cut is a launch of its own: ids from 0, XCD = id mod 8
            kb = len(side) // len(shapes)
            if len(side) == 0:
                continue
            assert len(side) == kb * len(shapes)
            for xcd in range(8):
                npos = side[xcd::8, 3]
                assert (np.diff(npos) <= 0).all(), (name, xcd, npos.tolist())
            # the plane blocks of a set in a row on one XCD (8 ids apart) where the counts divide, as before
            if len(side) % (8 * kb) == 0:
                for q in range(len(side) - 8):
                    if (q // 8) % kb != kb - 1 and side[q, 3] > 0:
                        assert (side[q + 8, :2] == side[q, :2]).all() and side[q + 8, 2] == side[q, 2] + COS_ZB, (name, q)
        sizes = [a * b for a, b in shapes]
        if sizes != sorted(sizes, reverse=True):
            reordered += 1
    # the order is not the coset order wherever a grid has blocks of more than one size: base_nz32 has 33 and 30 positions, and its cosets alternate
    sizes = [a * b for a, b in R.block_shapes(F.CASES["base_nz32"]["n"], (True, True))]
    assert {33, 30} <= set(sizes) and sizes != sorted(sizes, reverse=True) and reordered >= 1
    far, near = planner_records("base_nz32")
    first = far if len(far) else near
    assert first[0, 3] == 33 and np.concatenate([far, near])[-1, 3] in (30, 0)
    few = {a * b for a, b in R.block_shapes(F.CASES["few_tiles_12x30"]["n"], (True, True)) if a * b > 0}
    assert few == {5}


def test_the_variant_name_can_say_nosort_only_in_developer_builds():
    lib = os.path.join(ROOT, "openlifu-python_amd", "lib")
    with open(os.path.join(lib, "libolx.so"), "rb") as f:
        assert b",nosort" not in f.read()
    dbg = os.path.join(lib, "libolx_dbg.so")
    assert os.path.exists(dbg), "build() makes the debug library"
    with open(dbg, "rb") as f:
        debug = f.read()
    assert PIN.encode() in debug and b",nosort" in debug


# ---- GPU ----
_PRODUCT = {}
_REF = {}


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


def reference(case):
    """|p| of every focus from the fp64 C oracle with the steering the product solved, once per session."""
    if case not in _REF:
        _, _, (cs, pos_m, area, foci, d, ap, (xs, ys, zs)) = product_launch(case)
        _REF[case] = [np.abs(co.field_on_grid(xs, ys, zs, pos_m, area, d[f], ap[f], F.F0, F.C, F.P0, dmin=0.5e-3, absorption=cs.get("absorb", 0.0))) for f in range(len(d))]
    return _REF[case]


def worst_error(p, ref):
    worst = 0.0
    for f in range(len(ref)):
        assert np.isfinite(p[f]).all()
        worst = max(worst, np.abs(p[f].reshape(ref[f].shape) - ref[f]).max() / ref[f].max())
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("case", NAMES)
def test_volume_matches_the_oracle(case):
    """(a) Full-volume |p| of every focus against the fp64 C oracle with the product's launch (the position sets heaviest first)."""
    name, p, (cs, *_rest) = product_launch(case)
    assert "field_cosetp_k<nt2" in name and cs["expect"] in name and "nosort" not in name, name
    if cs["e4m3"] is not None:
        assert ("fp8corr" in name) == cs["e4m3"], name
    tol = R.FP8_BOUND if "fp8corr" in name else R.TOL_P
    worst = worst_error(p, reference(case))
    print(f"{case}: {name.strip()[:90]} | worst |p| error {worst:.3e} of the volume maximum (gate {tol:.1e})")
    assert worst <= tol, (case, worst)


_CHILD = r"""
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
from openlifu_amd import _native as nat
import test_gpu_cosetp_heavy_first as T
F = T.F
out = %r
assert "libolx_dbg" in os.path.basename(nat.LIB_PATH), nat.LIB_PATH
for case in T.NAMES:
    ctx = nat.Context(0)
    cs, pos_m, area, foci, d, ap, coords = F.prepare(ctx, case)
    for k in (T.PIN, "OLX_FP8_CORRECTION"):
        os.environ.pop(k, None)
    if cs.get("force"):
        os.environ["OLX_FP8_CORRECTION"] = "1"
    name, heavy = F.launch(ctx, cs, coords)
    os.environ[T.PIN] = "1"
    name_pin, coset = F.launch(ctx, cs, coords)
    for k in (T.PIN, "OLX_FP8_CORRECTION"):
        os.environ.pop(k, None)
    for nm in (name, name_pin):
        assert "field_cosetp_k<nt2" in nm and cs["expect"] in nm, nm
        if cs.get("force") or cs["e4m3"]:      # the e4m3 K-step body
            assert "fp8corr" in nm, nm
    assert ",nosort>" in name_pin and "nosort" not in name, (name, name_pin)      # the pin was honoured: the two launches walk the records in different orders
    ctx.sync()          # the debug library reports accesses outside their extent here
    ctx.close()
    if not (np.array_equal(heavy, coset) and np.isfinite(heavy).all() and heavy.max() > 0):
        print("DIFFERS:", case, name)
        sys.exit(3)
    np.save(os.path.join(out, case + ".npy"), heavy)
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
        out = str(tmp_path_factory.mktemp("heavy_first_dbg"))
        lib = os.path.join(ROOT, "openlifu-python_amd", "lib", "libolx_dbg.so")
        env = dict(os.environ, OLX_LIB_PATH=lib)
        for k in ("OLX_FIELD_VARIANT", "OLX_FP8_CORRECTION", "OLX_EXP_KGRP", "OLX_INTENSITY_STORED", "OLX_EXP_CP_NOREUSE", F.PIN, PIN):
            env.pop(k, None)
        code = _CHILD % (ROOT, os.path.join(ROOT, "openlifu-python_amd"), os.path.join(ROOT, "tests"), out)
        r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
        _DEBUG["run"] = (r.returncode, (r.stdout + r.stderr)[-3000:], out)
    return _DEBUG["run"]


@pytest.mark.gpu
def test_debug_library_reports_nothing_and_both_orders_have_the_bits_of_the_product(tmp_path_factory):
    """(b), (c): every instrumented index inside its extent in either order of the records; bit-identical |p| with and without OLX_EXP_CP_NOSORT=1;
    then the child's volumes against the product library's where the two run the same products (a forced-e4m3 case differs from the product's fp16
    corrections by design: its volume meets the oracle in the test below)."""
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
    assert compared >= len(NAMES) - len(FORCED)


@pytest.mark.gpu
@pytest.mark.parametrize("case", FORCED)
def test_forced_e4m3_volume_of_the_debug_library_matches_the_oracle(case, tmp_path_factory):
    """(a) for the e4m3 body where the planner may keep it off the grid (ragged nz; the e4m3 + clamp instantiation): the debug library's launch with
    the e4m3 products forced must name them, and its |p| volumes meet the fp64 C oracle at the gate of a variant that says fp8corr."""
    code, tail, out = debug_launches(tmp_path_factory)
    assert code == 0, (code, tail)
    with open(os.path.join(out, case + ".txt")) as fh:
        name = fh.read()
    cs = F.CASES[case]
    assert "field_cosetp_k<nt2" in name and "fp8corr" in name and cs["expect"] in name and "nosort" not in name, name
    _, _, (_, _, _, foci, d, ap, _) = product_launch(case)
    steer = np.load(os.path.join(out, case + "_steer.npz"))
    assert np.array_equal(steer["d"], d) and np.array_equal(steer["ap"], ap)      # the child solved the same steering: the reference is shared
    p = np.load(os.path.join(out, case + ".npy"))
    assert len(p) == len(foci)
    worst = worst_error(p, reference(case))
    print(f"{case} (debug library, e4m3 forced): {name.strip()[:90]} | worst |p| error {worst:.3e} of the volume maximum (gate {R.FP8_BOUND:.1e})")
    assert worst <= R.FP8_BOUND, (case, worst)
