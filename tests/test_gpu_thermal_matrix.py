"""Parity matrix of kernel 3 (k_thermal.hip: thermal_pack_k, thermal_step_k<UNI>, thermal_trace_k) against the fp64 oracle of the same
discrete scheme (tests/thermal_oracle.py), through the C-ABI wrapper (thermal_plan / _schedule / _source / _run / _fetch).

One table, CASES: every row has at most a few thousand voxels and names the kernel form it must reach ("uni": thermal_step_k<true>, no
coefficient volume; "het": thermal_pack_k with four volumes and thermal_step_k<false>; "het-mixed:<volumes>": thermal_pack_k with the other
pointers null).  test_table_reaches_every_form_and_edge spells out, by loops over the table, which paths and edges the rows must cover.

Gate, per case, computed on the CPU for that case and never from the kernel: with e32 the error of the oracle's own fp32 restatement
(thermal_oracle.run32) against the fp64 run,
    tol_rise = max(8 e32_rise, 1e-6)  of the oracle's maximum rise, for rise_max and every trace row,
    tol_cem  = max(8 e32_cem, 2e-5)   relative, wherever CEM43 > 1e-3 of its maximum.
The factor 8 covers what the restatement cannot copy (fused multiply-add contraction, the hardware exp2f, the order of the six face terms,
the conductances formed in fp32); the floors keep a lucky restatement from setting an unattainable gate.  Caps, as conditions on every row:
tol_rise <= 1e-5 and tol_cem <= 5e-4 (long_run_5000: 1e-3, written in its row: CEM43 is an fp32 running sum of 5000 terms).
test_sensitivity proves on the CPU that every named slip of thermal_oracle.PERTURBATIONS leaves the oracle by >= 10 gates at the row named
for it.  The media volumes and the source volumes are float32 values on both sides (the device and the oracle get the same numbers).

Measured on one MI355X, worst over the table (the restatement's value of the same row beside it):
    rise_max and traces        2.05e-07 of the maximum (het_axes_1x1x1; restatement 1.14e-07, gate 1.00e-06); all rows 0.4e-7 ... 2.1e-7
    CEM43, rows of <= 300 steps 2.22e-06 relative (het_mixed_alpha; restatement 2.60e-06, gate 2.08e-05)
    CEM43, heat_then_cool (600) 1.72e-05 (restatement 1.71e-05, gate 1.36e-04)
    CEM43, long_run_5000        7.23e-05 (restatement 7.23e-05, gate 5.79e-04): the growth of the fp32 sum, the same on both sides
    the PII source              9.18e-08 / 6.69e-07 (restatement 8.83e-08 / 8.64e-07)
    dt_max                      the fp64 formula of the uniform rows equal to the oracle's, the packed rows within 8.3e-08 relative
No row needs more than the factor 8: the device stays within 3 times its row's restatement everywhere.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from openlifu_amd import _native as nat
import thermal_oracle as to
from test_gpu_thermal import WATER, SKULL, TISSUE, _np_m, gaussian_sources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "openlifu-python_amd", "lib")
MATS = np.array([WATER, SKULL, TISSUE])
QUANT = ("rho", "cp", "kappa", "alpha")
H_ISO = (0.5e-3,) * 3
H_ANISO = (0.4e-3, 0.5e-3, 0.3e-3)
MIXED = ("kappa", "alpha", "rho,cp", "rho,kappa,alpha", "cp")
FACES = tuple(f"noface{a}{s}" for a in range(3) for s in "+-")


def _case(id, form, shape, h, peak, centres=None, perfusion=0.0, baseline=37.0, steps=150, dt_frac=1.0, sched="mod4", extra_points=(),
          cem_cap=5e-4, names=(), corners=False):
    if centres is None:
        centres = [tuple(s // 2 for s in shape)]
    return dict(id=id, form=form, shape=tuple(shape), h=h, peak=peak, centres=[tuple(c) for c in centres], perfusion=perfusion,
                baseline=baseline, steps=steps, dt_frac=dt_frac, sched=sched, extra_points=tuple(extra_points), cem_cap=cem_cap,
                names=tuple(names), corners=corners)


def _table():
    t = [
        # heat reaches all six faces of the uniform kernel, with perfusion and three different spacings
        _case("uni_aniso_perf_corners", "uni", (13, 9, 21), H_ANISO, 3000.0, [(0, 0, 0), (12, 8, 20), (6, 4, 10)], perfusion=2e4, steps=300,
              names=FACES + ("swapyz_minus", "noperf", "rowshift", "cemlag"), corners=True),
        # ... and of the packed kernel: every inner face a harmonic mean of unequal kappa; 41 degC, so both branches of R
        _case("het_random_corners", "het", (9, 8, 11), H_ANISO, 300.0, [(0, 0, 0), (8, 7, 10), (4, 4, 5)], perfusion=2e4, baseline=41.0,
              steps=300, names=("arith",) + FACES + ("swapyz_minus", "s_uniform", "noperf", "rowshift", "cemlag"), corners=True),
        _case("het_random_corners_half", "het", (9, 8, 11), H_ANISO, 300.0, [(0, 0, 0), (8, 7, 10), (4, 4, 5)], baseline=41.0, steps=300,
              dt_frac=0.5, corners=True),
    ]
    # thermal_pack_k with some pointers null: the rest are TISSUE's scalars
    t += [_case(f"het_mixed_{m.replace(',', '_')}", f"het-mixed:{m}", (6, 5, 7), H_ANISO, 1000.0, [(0, 0, 0), (5, 4, 6), (3, 2, 3)], perfusion=2e4)
          for m in MIXED]
    # axes of length 1 (no inner face along them), a single voxel, the smallest grid with every voxel on three boundary faces
    for shape in ((1, 1, 1), (1, 1, 300), (300, 1, 1), (1, 257, 1), (2, 2, 2)):
        tag = "x".join(str(s) for s in shape)
        t.append(_case(f"uni_axes_{tag}", "uni", shape, H_ISO, 3000.0))
        t.append(_case(f"het_axes_{tag}", "het", shape, H_ISO, 300.0))
    # 960 and 1365 voxels: a partial last block, a partial last wave; 44 degC: the upper branch of R from the first step
    for shape in ((5, 3, 64), (3, 7, 65)):
        tag = "x".join(str(s) for s in shape)
        t.append(_case(f"uni_tail_{tag}", "uni", shape, H_ANISO, 3000.0, perfusion=2e4, baseline=44.0))
        t.append(_case(f"het_tail_{tag}", "het", shape, H_ANISO, 300.0, perfusion=2e4, baseline=44.0))
    t += [
        # the last step is a third of the answer: a rise or CEM43 record taken before the step shows
        _case("short_run_3_steps", "het", (6, 5, 7), H_ANISO, 300.0, steps=3, sched="on", names=("riselag",)),
        _case("short_run_3_steps_uni", "uni", (6, 5, 7), H_ANISO, 4000.0, steps=3, sched="on"),
        # the source is on for the first 200 steps only: rise_max is not the final state, the traces gate the cooling
        _case("heat_then_cool", "het", (4, 3, 32), H_ANISO, 150.0, perfusion=2e4, baseline=40.0, steps=600, dt_frac=0.9, sched="on200"),
        # the growth of the fp32 CEM43 sum with the step count; cap 1e-3 instead of 5e-4: 8 x 6.6e-5 on the CPU
        _case("long_run_5000", "het", (4, 3, 32), H_ANISO, 40.0, perfusion=2e4, baseline=40.0, steps=5000, dt_frac=0.9, sched="on", cem_cap=1e-3),
        # more than 256 trace points, duplicates included: the stride loop of thermal_step_k's block 0, two blocks of thermal_trace_k
        _case("points_over_one_block", "het", (6, 5, 7), H_ANISO, 150.0, perfusion=2e4, extra_points=tuple(range(210)) + tuple(range(0, 180, 2))),
    ]
    return t


CASES = _table()
BY_ID = {c["id"]: c for c in CASES}
IDS = [c["id"] for c in CASES]


def volumes_of(form):
    """the media that are volumes in a row of this form"""
    if form == "uni":
        return ()
    if form == "het":
        return QUANT
    assert form.startswith("het-mixed:"), form
    return tuple(form.split(":", 1)[1].split(","))


def medium_of(c):
    """(rho, cp, kappa, alpha [Np/m]): float32-valued volumes (random labels of WATER / SKULL / TISSUE per voxel) or TISSUE's scalars"""
    vols = volumes_of(c["form"])
    lab = np.random.default_rng(sum(c["shape"]) + len(vols)).integers(0, 3, c["shape"])
    out = []
    for qi, q in enumerate(QUANT):
        if q in vols:
            v = _np_m(MATS[lab, qi]) if q == "alpha" else MATS[lab, qi]
            out.append(v.astype(np.float32).astype(np.float64))
        else:
            out.append(float(_np_m(TISSUE[qi])) if q == "alpha" else float(TISSUE[qi]))
    return tuple(out)


def schedule_of(c, dt, F):
    """CSR (row_ptr, focus, tau).  "mod4": row n has n % 4 entries (so empty rows occur), a third entry repeats the second entry's focus,
    tau = dt (0.3 + 0.2 j), and every seventh row that has entries ends with a tau = 0 entry.  "on": focus 0 for the whole of every
    step; "on200": the same for the first 200 steps, nothing after."""
    rows = []
    for n in range(c["steps"]):
        if c["sched"] == "mod4":
            ent = [((n + min(j, 1)) % F, dt * (0.3 + 0.2 * j)) for j in range(n % 4)]
            if n % 7 == 0 and ent:
                ent[-1] = (ent[-1][0], 0.0)
        else:
            ent = [(0, dt)] if c["sched"] == "on" or n < 200 else []
        rows.append(ent)
    row_ptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
    focus = np.array([f for r in rows for f, _ in r], dtype=np.int32)
    tau = np.array([x for r in rows for _, x in r], dtype=np.float64)
    return row_ptr, focus, tau


def points_of(c):
    vox = int(np.prod(c["shape"]))
    return np.array([0, vox - 1] + [int(np.ravel_multi_index(p, c["shape"])) for p in c["centres"]] + list(c["extra_points"]), dtype=np.int64)


def oracle_bound(c):
    rho, cp, kap, _ = medium_of(c)
    return float(to.ftcs_bound(rho, cp, kap, c["h"], c["shape"], c["perfusion"]))


_REF = {}


def reference(c, dt_max, inten=None, tau_scale=1.0):
    """The fp64 run, its fp32 restatement's error and the gate of a row at dt = dt_frac dt_max; computed once per (row, dt) and shared."""
    key = (c["id"], dt_max, tau_scale)
    if key not in _REF:
        dt = c["dt_frac"] * dt_max
        if inten is None:
            inten = gaussian_sources(c["shape"], c["centres"], 1.5, peak=c["peak"])
        rp, fo, tau = schedule_of(c, dt, inten.shape[0])
        args = medium_of(c) + (inten, c["h"], rp, fo, tau * tau_scale, dt, c["steps"])
        kw = dict(baseline=c["baseline"], perfusion=c["perfusion"], points=points_of(c))
        ref, r32 = to.run(*args, **kw), to.run32(*args, **kw)
        e32_rise, e32_cem = errors(r32, ref)
        for a in ref:
            a.setflags(write=False)
        _REF[key] = dict(ref=ref, args=args, kw=kw, dt=dt, e32_rise=e32_rise, e32_cem=e32_cem, tol_rise=max(8 * e32_rise, 1e-6),
                         tol_cem=max(8 * e32_cem, 2e-5))
    return _REF[key]


def errors(got, ref):
    """(rise_max and trace error over the oracle's maximum rise, CEM43 relative error wherever it exceeds 1e-3 of its maximum)"""
    scale = float(ref[0].max())
    e = float(np.abs(got[0] - ref[0]).max())
    if ref[2].size:
        assert got[2].shape == ref[2].shape, (got[2].shape, ref[2].shape)
        e = max(e, float(np.abs(got[2] - ref[2]).max()))
    m = ref[1] > 1e-3 * ref[1].max()
    return e / scale, float((np.abs(got[1][m] - ref[1][m]) / ref[1][m]).max())


# ---- CPU: the table is what it says, the reference stands alone, the gate sees every named slip ----------------------------------
def test_table_reaches_every_form_and_edge():
    assert len(set(IDS)) == len(IDS)
    forms = {c["form"] for c in CASES}
    assert {"uni", "het"} <= forms
    for m in MIXED:
        assert f"het-mixed:{m}" in forms, m
        assert 0 < len(volumes_of(f"het-mixed:{m}")) < 4
    for form in ("uni", "het"):
        rows = [c for c in CASES if c["form"] == form]
        assert any(c["perfusion"] == 0 for c in rows) and any(c["perfusion"] > 0 for c in rows), form
        assert any(len(set(c["h"])) == 1 for c in rows) and any(len(set(c["h"])) == 3 for c in rows), form
        for a in range(3):
            assert any(c["shape"][a] == 1 and max(c["shape"]) > 1 for c in rows), (form, a)
        vox = [int(np.prod(c["shape"])) for c in rows]
        assert any(v % 64 for v in vox) and any(v % 256 and v > 256 for v in vox) and any(v < 64 for v in vox), form
        assert any(v > 256 and v % 64 == 0 and v % 256 for v in vox), form       # whole waves, a partial last block
    empty = three = repeat = tau0 = False
    for c in CASES:
        assert int(np.prod(c["shape"])) <= 4096, c["id"]
        assert all(0 <= p[a] < c["shape"][a] for p in c["centres"] for a in range(3)), c["id"]
        if c["form"] != "het":
            continue
        rp, fo, tau = schedule_of(c, 1.0, len(c["centres"]))
        for n in range(c["steps"]):
            f = list(fo[rp[n]:rp[n + 1]])
            empty |= len(f) == 0
            three |= len(f) >= 3
            repeat |= len(set(f)) < len(f)
            tau0 |= bool((tau[rp[n]:rp[n + 1]] == 0).any())
    assert empty and three and repeat and tau0
    assert any(len(points_of(c)) > 256 and len(set(points_of(c))) < len(points_of(c)) for c in CASES)
    assert any(c["baseline"] >= 43.0 for c in CASES)
    crossing = [c for c in CASES if c["baseline"] < 43.0 and c["baseline"] + reference(c, oracle_bound(c))["ref"][0].max() > 43.0]
    assert crossing and any(c["form"] == "het" for c in crossing)
    assert any(c["steps"] <= 3 for c in CASES) and any(c["steps"] >= 5000 for c in CASES)


@pytest.mark.parametrize("cid", IDS)
def test_reference_alone(cid):
    c = BY_ID[cid]
    r = reference(c, oracle_bound(c))
    rise, cem, traces, final = r["ref"]
    print(f"[thermal] {cid}: rise_max {rise.max():.3g} K, restatement rise {r['e32_rise']:.2e} cem43 {r['e32_cem']:.2e}, "
          f"gate {r['tol_rise']:.2e} / {r['tol_cem']:.2e}")
    assert np.isfinite(rise).all() and np.isfinite(cem).all() and rise.max() > 0
    assert rise.max() < 60.0, rise.max()                        # stable at this dt, and a temperature fp32 exp2f can take
    assert (cem > 1e-3 * cem.max()).sum() >= 1
    # the restatement passes the gate by the factor 8, and the gate is within the caps
    assert 8 * r["e32_rise"] <= r["tol_rise"] <= 1e-5, (r["e32_rise"], r["tol_rise"])
    assert 8 * r["e32_cem"] <= r["tol_cem"] <= c["cem_cap"], (r["e32_cem"], r["tol_cem"])
    assert c["cem_cap"] == (1e-3 if cid == "long_run_5000" else 5e-4)
    if c["corners"]:                                             # heat does reach every face
        for a in range(3):
            for side in (0, -1):
                assert np.abs(np.take(final, side, axis=a)).max() > 1e-3 * final.max(), (a, side)
    if c["sched"] == "on200":                                    # it cools: the maximum was reached before the end
        assert final.max() < 0.9 * rise.max()


SENSITIVE = [(c["id"], p) for c in CASES for p in c["names"]]


@pytest.mark.parametrize("cid,pert", SENSITIVE)
def test_sensitivity(cid, pert):
    c = BY_ID[cid]
    r = reference(c, oracle_bound(c))
    moved_rise, moved_cem = errors(to.run(*r["args"], **r["kw"], pert=pert), r["ref"])
    print(f"[thermal] {cid} / {pert}: moves rise {moved_rise:.2e} ({moved_rise / r['tol_rise']:.0f} gates), "
          f"cem43 {moved_cem:.2e} ({moved_cem / r['tol_cem']:.0f} gates)")
    assert moved_rise >= 10 * r["tol_rise"] or moved_cem >= 10 * r["tol_cem"], (moved_rise, moved_cem)


def test_every_perturbation_is_named():
    assert set(to.PERTURBATIONS) == {p for _, p in SENSITIVE}
    with pytest.raises(ValueError):
        to.run(*reference(BY_ID["uni_axes_1x1x1"], oracle_bound(BY_ID["uni_axes_1x1x1"]))["args"], pert="no_such_slip")


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    c = nat.Context(0)
    yield c
    c.close()


def plan(ctx, c):
    """-> the device's dt_max of the row's grid and medium"""
    return ctx.thermal_plan((0.0, 0.0, 0.0), c["h"], c["shape"], *medium_of(c), perfusion=c["perfusion"])


def stage(ctx, c, r):
    """schedule and source of a planned row, from its reference's inputs"""
    inten, _, rp, fo, tau = r["args"][4:9]
    ctx.thermal_schedule(rp, fo, tau, points=r["kw"]["points"])
    ctx.thermal_source(inten.shape[0], inten)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", IDS)
def test_matrix_case(ctx, cid):
    c = BY_ID[cid]
    r = reference(c, plan(ctx, c))                 # dt is the bound the device returned, times the row's fraction
    stage(ctx, c, r)
    ctx.thermal_run(r["dt"], c["baseline"])
    got = ctx.thermal_fetch()
    e_rise, e_cem = errors(got, r["ref"])
    print(f"[thermal] {cid} ({c['form']}): rise {e_rise:.2e} (restatement {r['e32_rise']:.2e}, gate {r['tol_rise']:.2e}), "
          f"cem43 {e_cem:.2e} (restatement {r['e32_cem']:.2e}, gate {r['tol_cem']:.2e})")
    assert r["tol_rise"] <= 1e-5 and r["tol_cem"] <= c["cem_cap"]
    assert e_rise <= r["tol_rise"], (e_rise, r["tol_rise"])
    assert e_cem <= r["tol_cem"], (e_cem, r["tol_cem"])


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["het_random_corners", "uni_aniso_perf_corners"])
def test_continued_runs_are_the_single_run(ctx, cid):
    c = BY_ID[cid]
    r = reference(c, plan(ctx, c))
    stage(ctx, c, r)
    dt, b, n = r["dt"], c["baseline"], c["steps"]
    ctx.thermal_run(dt, b)
    one = ctx.thermal_fetch()
    assert one[2].shape == (n, len(r["kw"]["points"])) and one[0].max() > 0
    ctx.thermal_run(dt, b, 0, 1)
    ctx.thermal_run(dt, b, 1, 63)
    part = ctx.thermal_fetch()
    assert part[2].shape[0] == 64 and np.array_equal(part[2], one[2][:64])
    ctx.thermal_run(dt, b, 64, 0)                  # no step: nothing changes, the run stays continuable
    assert all(np.array_equal(x, y) for x, y in zip(ctx.thermal_fetch(), part))
    with pytest.raises(nat.NativeError, match=r"olx -2.*does not continue"):      # OLX_ESTATE
        ctx.thermal_run(dt, b, 70, 10)
    ctx.thermal_run(dt, b, 64, n - 64)
    split = ctx.thermal_fetch()
    for name, x, y in zip(("rise_max", "cem43", "traces"), split, one):            # same kernels, same inputs, same order
        assert np.array_equal(x, y), name
    ctx.thermal_run(dt, b, 0, 0)
    rise, cem, tr = ctx.thermal_fetch()
    assert tr.shape[0] == 0 and not rise.any() and not cem.any()


@pytest.mark.gpu
def test_device_bound_matches_oracle(ctx):
    for c in CASES:
        dev, ref = plan(ctx, c), oracle_bound(c)
        rel = abs(dev - ref) / ref
        print(f"[thermal] {c['id']} ({c['form']}): dt_max {dev:.9g} s, oracle {ref:.9g} s, rel {rel:.2e}")
        # uniform: an fp64 host formula; packed: about a dozen fp32 roundings of 6e-8, the maximum taken exactly through the bit pattern
        assert rel <= (1e-12 if c["form"] == "uni" else 2e-6), (c["id"], rel)
        ctx.thermal_schedule([0, 1], [0], [0.5 * dev])
        ctx.thermal_source(1, np.ones((1,) + c["shape"], dtype=np.float32))
        ctx.thermal_run(dev, 37.0)
        with pytest.raises(ValueError, match="above the FTCS bound"):
            ctx.thermal_run(1.001 * dev, 37.0)


@pytest.mark.gpu
def test_pii_source_matches_oracle():
    """The resident pulse intensity integrals read in place as the source (olx_pii_upload, olx_thermal_source_pii)."""
    c = BY_ID["het_random_corners"]
    pii = (gaussian_sources(c["shape"], c["centres"], 1.5, peak=c["peak"]) * np.float32(2.3e-5)).astype(np.float32)   # [J/cm^2] of 23 us pulses
    own = nat.Context(0)
    try:
        own.field_upload((0.0, 0.0, 0.0), c["h"], c["shape"], np.ones_like(pii))
        own.pii_upload(pii)
        r = reference(c, plan(own, c), inten=pii, tau_scale=1.0 / 2.3e-5)
        _, _, rp, fo, tau = r["args"][4:9]
        own.thermal_schedule(rp, fo, tau, points=r["kw"]["points"])
        own.thermal_source_pii(pii.shape[0])
        own.thermal_run(r["dt"], c["baseline"])
        got = own.thermal_fetch()
        assert np.array_equal(own.pii_fetch(pii.shape[0]), pii)            # read in place, unchanged
    finally:
        own.close()
    e_rise, e_cem = errors(got, r["ref"])
    print(f"[thermal] pii source: rise {e_rise:.2e} (restatement {r['e32_rise']:.2e}, gate {r['tol_rise']:.2e}), "
          f"cem43 {e_cem:.2e} (restatement {r['e32_cem']:.2e}, gate {r['tol_cem']:.2e})")
    assert r["ref"][0].max() > 1.0 and r["tol_rise"] <= 1e-5 and r["tol_cem"] <= 5e-4
    assert e_rise <= r["tol_rise"] and e_cem <= r["tol_cem"], (e_rise, e_cem)


BAD = [(q, v) for q in QUANT for v in (np.nan, np.inf, 0.0, -1.0) if not (q == "alpha" and v == 0.0)]
BAD_NAME = dict(rho="density", cp="specific heat", kappa="conductivity", alpha="absorption")


@pytest.mark.gpu
def test_thermal_plan_refuses_bad_media(ctx):
    """One bad voxel in the middle of a sane volume, so that its wave holds sane lanes: refused by name, the standing plan untouched."""
    c = dict(BY_ID["het_random_corners"], steps=40)
    dt_max = plan(ctx, c)
    r = reference(dict(c, id="het_random_corners_40"), dt_max)
    stage(ctx, c, r)
    ctx.thermal_run(r["dt"], c["baseline"])
    base = ctx.thermal_fetch()
    assert base[0].max() > 0
    mid = tuple(s // 2 for s in c["shape"])
    accepted = []
    for q, bad in BAD:
        med = [np.array(m) for m in medium_of(c)]
        med[QUANT.index(q)][mid] = bad
        try:
            ctx.thermal_plan((0.0, 0.0, 0.0), c["h"], c["shape"], *med, perfusion=c["perfusion"])
            accepted.append((q, bad))
            print(f"[thermal] a {q} volume with one voxel = {bad} was accepted")
            break                                   # (that plan replaced the standing one: nothing more to learn from this context)
        except ValueError as e:
            assert "olx_thermal_plan" in str(e) and BAD_NAME[q] in str(e), str(e)
        ctx.thermal_run(r["dt"], c["baseline"])    # the plan, schedule and source of before still stand
        again = ctx.thermal_fetch()
        assert all(np.array_equal(x, y) for x, y in zip(again, base)), (q, bad)
    assert not accepted, accepted
    # alpha = 0 is legal
    med = [np.array(m) for m in medium_of(c)]
    med[3][mid] = 0.0
    assert ctx.thermal_plan((0.0, 0.0, 0.0), c["h"], c["shape"], *med, perfusion=c["perfusion"]) == pytest.approx(dt_max, rel=1e-12)


@pytest.mark.gpu
def test_matrix_stays_inside_its_extents_in_the_debug_library():
    """The matrix and the continued runs against libolx_dbg.so (every index of kernel 3 counted against its extent), in one child process.
    long_run_5000 stays out of the child: its two CPU references alone take longer than the rest of the selection."""
    env = dict(os.environ, OLX_LIB_PATH=os.path.join(LIB, "libolx_dbg.so"))
    sel = "(test_matrix_case and not long_run_5000) or test_continued_runs"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", sel, "-p", "no:cacheprovider"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in tail and "failed" not in tail, tail
