"""Pulsed (tone-burst) field model on the MI355X: kernel 2p (field_pulse_k) through the C-ABI against the fp64 oracle
(tests/pulsed_oracle.py), its limits and invariants, and Protocol.calc_solution with SimSetup.options["field_model"] = "pulsed".
Gate: error <= 1e-5 of the volume maximum for p_max and p_min, voxels whose t_e / dt or (t_e + T) / dt lies
within 1e-7 of an integer excluded (fewer than 0.1 % of them)."""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

import openlifu_amd as ol
from openlifu_amd import _native as nat
from openlifu_amd.sim import field as sf
from oracle import bf_oracle as bo
from conftest import centred_grid, synthetic_array
import pulsed_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "openlifu-python_amd", "lib")
F0, C, RHO, P0 = 400e3, 1500.0, 1000.0, 1e5
TOL, MARGIN, MAX_EXCLUDED = 1e-5, 1e-7, 1e-3
# grids shifted off the lattice that c dt and the element pitch span: on it, whole families of voxels have t_e / dt EXACTLY on an integer
# (Pythagorean quadruples of the index differences), where fp64 rounding alone decides whether a term is in or out of a sample
SHIFT = np.array([0.0731, -0.0419, 0.0263]) * 1e-3


def linear_array(n=64, pitch_mm=0.5):
    pos = np.zeros((n, 3))
    pos[:, 0] = (np.arange(n) - (n - 1) / 2) * pitch_mm
    size = np.tile([0.9 * pitch_mm, 10.0], (n, 1))
    return pos, np.zeros_like(pos), size


def run_kernel(ctx, pos_mm, size, foci_mm, xs, ys, zs, cycles, dt=0.0, t_end=0.0, cfl=0.5, absorption=0.0, delays=None):
    """(outputs dict, delays, apod, area, pos_m, dt, n_t) of one pulsed launch with the oracle's steering."""
    pos_m = pos_mm * 1e-3
    area = size[:, 0] * size[:, 1] * 1e-6
    ctx.set_elements(pos_m, np.tile([0.0, 0.0, 1.0], (len(pos_m), 1)), area)
    if delays is None:
        steer = [bo.beamform(pos_m, np.zeros_like(pos_m), f, C) for f in np.atleast_2d(foci_mm) * 1e-3]
        delays, apod = np.array([s[0] for s in steer]), np.array([s[1] for s in steer])
    else:
        apod = np.ones_like(delays)
    ctx.set_steering(delays, apod)
    sp = [xs[1] - xs[0], ys[1] - ys[0], zs[1] - zs[0]]
    n = (len(xs), len(ys), len(zs))
    dt, n_t = sf.pulse_time_axis(sp, n, dt, t_end, cfl)
    ctx.field_absorption(absorption)
    ctx.field_pulse(cycles, dt, n_t)
    try:
        ctx.field_plan((xs[0], ys[0], zs[0]), sp, n, F0, C, RHO, P0, flags=nat.OUT_PMAG | nat.OUT_INTENSITY | nat.OUT_PMAX)
        ctx.field_launch()
        out = ctx.field_fetch_all(want=("pmag", "intensity", "pmax"))
        ctx.sync()
    finally:
        ctx.field_pulse(0.0, 0.0, 0)
        ctx.field_absorption(0.0)
    return out, delays, apod, area, pos_m, dt, n_t


def oracle_grid(xs, ys, zs, pos_m, area, delays, apod, cycles, dt, n_t, absorption=0.0):
    return [po.pulsed_grid(xs, ys, zs, pos_m, area, delays[f], apod[f], F0, C, P0, cycles, dt, n_t, absorption) for f in range(len(delays))]


def check_gate(out, ref):
    """Per focus: max error of p_max / p_min over the included voxels <= 1e-5 of the oracle's volume maximum; returns the errors."""
    errs = []
    for f, (omax, omin, margin) in enumerate(ref):
        ok = margin >= MARGIN
        assert (~ok).mean() < MAX_EXCLUDED, f"{(~ok).mean():.2e} of the voxels excluded"
        for gpu, o, name in ((out["pmax"][f], omax, "p_max"), (out["pmag"][f], omin, "p_min")):
            e = np.abs(gpu.astype(np.float64) - o)[ok].max() / o.max()
            assert e <= TOL, f"focus {f} {name}: error {e:.3e} of the volume maximum"
            errs.append(e)
        it = 1e-4 * out["pmag"][f].astype(np.float64) ** 2 / (2 * RHO * C)
        assert np.allclose(out["intensity"][f], it, rtol=1e-5, atol=1e-7 * it.max())
    return errs


@pytest.fixture(scope="module")
def ctx():
    c = nat.Context(0)
    yield c
    c.close()


# ---- 6. kernel against the oracle, full volumes -----------------------------------------------------------------------------------
CASES = {
    "linear64_1focus": dict(arr="linear", foci=[[0, 0, 15.0]], n=(32, 32, 32), h=0.5, cycles=3, t_end=0.0, absorption=0.0),
    "linear64_8foci_absorbing": dict(arr="linear", foci=[[x, 0, z] for x in (-3.0, 0.0, 3.0, 5.0) for z in (12.0, 18.0)], n=(32, 32, 32),
                                     h=0.5, cycles=4, t_end=4e-5, absorption=2.5),
    "matrix16x16_1focus": dict(arr="matrix", foci=[[0, 0, 25.0]], n=(32, 32, 32), h=1.0, cycles=3, t_end=5e-5, absorption=0.0),
    "matrix16x16_odd_absorbing": dict(arr="matrix", foci=[[2.0, -1.0, 20.0]], n=(33, 31, 35), h=1.0, cycles=5, t_end=0.0, absorption=5.0),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_pulsed_kernel_matches_oracle_small(ctx, name):
    k = CASES[name]
    pos, _, size = linear_array() if k["arr"] == "linear" else synthetic_array(16, 16, 3.0)
    nx, ny, nz = k["n"]
    xs = (np.arange(nx) - (nx - 1) / 2) * k["h"] * 1e-3 + SHIFT[0]
    ys = (np.arange(ny) - (ny - 1) / 2) * k["h"] * 1e-3 + SHIFT[1]
    zs = (5.0 + np.arange(nz) * k["h"]) * 1e-3 + SHIFT[2]
    out, delays, apod, area, pos_m, dt, n_t = run_kernel(ctx, pos, size, k["foci"], xs, ys, zs, k["cycles"], t_end=k["t_end"],
                                                         absorption=k["absorption"])
    ref = oracle_grid(xs, ys, zs, pos_m, area, delays, apod, k["cycles"], dt, n_t, k["absorption"])
    check_gate(out, ref)
    if name == "linear64_1focus":
        # 12. p_max != p_min: the burst is short, the field is not a CW magnitude; where they differ the oracle agrees
        omax, omin, margin = ref[0]
        diff = np.abs(out["pmax"][0] - out["pmag"][0])
        sel = (diff > 1e-2 * omin.max()) & (margin >= MARGIN)
        assert sel.sum() > 100
        assert np.abs((out["pmax"][0] - out["pmag"][0])[sel] - (omax - omin)[sel]).max() <= 2 * TOL * max(omax.max(), omin.max())


# ---- 7. sampled voxels at full size --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_pulsed_kernel_matches_oracle_sampled_256(ctx):
    pos, _, size = synthetic_array(16, 16, 3.0)
    xs, ys, zs = centred_grid(256, 0.25)
    out, delays, apod, area, pos_m, dt, n_t = run_kernel(ctx, pos, size, [[0, 0, 35.0]], xs, ys, zs, cycles=20)
    rng = np.random.default_rng(2024)
    idx = rng.integers(0, 256, size=(20000, 3))
    pts = np.stack([xs[idx[:, 0]], ys[idx[:, 1]], zs[idx[:, 2]]], axis=1)
    omax, omin, margin = po.pulsed_points(pts, pos_m, area, delays[0], apod[0], F0, C, P0, 20, dt, n_t, 0.5 * 0.25e-3, chunk=128)
    ok = margin >= MARGIN
    assert (~ok).mean() < MAX_EXCLUDED
    vmax_p, vmax_n = out["pmax"][0].max(), out["pmag"][0].max()       # the volume maxima (the sample may miss the focus)
    gx, gn = out["pmax"][0][tuple(idx.T)], out["pmag"][0][tuple(idx.T)]
    assert np.abs(gx - omax)[ok].max() <= TOL * vmax_p
    assert np.abs(gn - omin)[ok].max() <= TOL * vmax_n
    assert omax.max() > 0.2 * vmax_p          # (the sample reaches into the beam)


# ---- 8. a window longer than one LDS pass --------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_pulsed_window_longer_than_one_pass(ctx):
    pos, _, size = synthetic_array(4, 4, 3.0)
    xs, ys, zs = (v + s for v, s in zip(centred_grid(16, 1.0), SHIFT))
    dt = 1.0 / (40 * F0)                       # 40 samples per period, 60 cycles: T / dt = 2400 > 1344 samples per pass
    out, delays, apod, area, pos_m, dt, n_t = run_kernel(ctx, pos, size, [[0, 0, 12.0]], xs, ys, zs, cycles=60, dt=dt, t_end=2e-4)
    assert 60 / (F0 * dt) > 64 * 21
    check_gate(out, oracle_grid(xs, ys, zs, pos_m, area, delays, apod, 60, dt, n_t))


# ---- 9. CW limit ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_pulsed_long_burst_approaches_cw(ctx):
    K = 16
    pos, _, size = synthetic_array(8, 8, 3.0)
    xs, ys, zs = centred_grid(32, 1.0)
    dt = 1.0 / (K * F0)
    out, delays, apod, area, pos_m, dt, n_t = run_kernel(ctx, pos, size, [[2.0, 0, 20.0]], xs, ys, zs, cycles=30, dt=dt, t_end=1e-4)
    # the CW kernel fed the truncated delays, three fp16 correction products pinned
    ctx.set_steering(sf.truncate_delays(delays, dt), apod)
    ctx.field_plan((xs[0], ys[0], zs[0]), [1e-3] * 3, (32, 32, 32), F0, C, RHO, P0, flags=nat.OUT_PMAG | nat.FIELD_FP16_CORRECTION)
    ctx.field_launch()
    cw = ctx.field_fetch_all(want=("pmag",))["pmag"][0]
    X, Y, Z = np.meshgrid(xs, ys, zs, indexing="ij")
    u, _ = po.arrival_steps(np.stack([X.ravel(), Y.ravel(), Z.ravel()], 1), pos_m, delays[0], dt, C, 0.5e-3)
    lo, hi = u.max(1), np.minimum((u + 30 * K).min(1), n_t - 1)
    full = (hi - lo >= K + 1).reshape(cw.shape)          # the full-overlap interval spans at least one period of samples
    assert full.mean() > 0.5
    tol = 1e-5 * cw.max()
    pm = out["pmax"][0]
    assert np.all(pm[full] >= np.cos(np.pi / K) * cw[full] - tol)
    # the upper bound holds where the steady state dominates; near CW nulls the partial sums of the rise and fall of the burst may
    # exceed the steady-state magnitude (the transients the pulsed model exists for)
    beam = full & (cw >= 0.5 * cw.max())
    assert beam.sum() > 10
    assert np.all(pm[beam] <= cw[beam] + tol)


# ---- 10. t_end truncation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_late_arrivals_give_exact_zero(ctx):
    pos, _, size = linear_array()
    xs, ys, zs = centred_grid(32, 1.0)
    out, delays, apod, area, pos_m, dt, n_t = run_kernel(ctx, pos, size, [[0, 0, 15.0]], xs, ys, zs, cycles=3, t_end=1.4e-5)
    X, Y, Z = np.meshgrid(xs, ys, zs, indexing="ij")
    u, _ = po.arrival_steps(np.stack([X.ravel(), Y.ravel(), Z.ravel()], 1), pos_m, delays[0], dt, C, 0.5e-3)
    late = (np.ceil(u.min(1) - 1e-7) >= n_t).reshape(out["pmax"][0].shape)
    assert 0.05 < late.mean() < 0.95
    for key in ("pmax", "pmag", "intensity"):
        assert np.all(out[key][0][late] == 0.0), key
    assert np.all(out["pmag"][0][~late] >= 0.0) and out["pmag"][0][~late].max() > 0


# ---- 11. delay truncation -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_half_step_shifted_delays_give_identical_volumes(ctx):
    pos, _, size = synthetic_array(8, 8, 3.0)
    xs, ys, zs = centred_grid(24, 1.0)
    steer = bo.beamform(pos * 1e-3, np.zeros_like(pos), np.array([1.0, -2.0, 18.0]) * 1e-3, C)
    dt, _ = sf.pulse_time_axis([1e-3] * 3, (24, 24, 24))
    a = run_kernel(ctx, pos, size, None, xs, ys, zs, cycles=4, delays=steer[0][None, :])[0]
    b = run_kernel(ctx, pos, size, None, xs, ys, zs, cycles=4, delays=((np.floor(steer[0] / dt) + 0.5) * dt)[None, :])[0]
    assert not np.array_equal(steer[0], (np.floor(steer[0] / dt) + 0.5) * dt)
    for key in ("pmax", "pmag", "intensity"):
        assert np.array_equal(a[key], b[key]), key


# ---- 13 / 14. Protocol.calc_solution ----------------------------------------------------------------------------------------------------
def _protocol(options):
    setup = ol.SimSetup(options=dict(options))
    return ol.Protocol(pulse=ol.Pulse(frequency=F0, duration=2e-5), sequence=ol.Sequence(pulse_count=4, pulse_train_interval=0),
                       focal_pattern=ol.focal_patterns.Wheel(center=True, num_spokes=3, spoke_radius=3.0, target_pressure=1e6),
                       sim_setup=setup, apod_method=ol.apod_methods.MaxAngle(max_angle=40.0))


def _array():
    return ol.Transducer.gen_matrix_array(nx=8, ny=8, pitch=4, kerf=0.4, units="mm", sensitivity=1e5)


@pytest.mark.gpu
def test_calc_solution_pulsed_end_to_end(tmp_path):
    target = ol.Point(position=(0, 0, 30), units="mm")
    sol, agg, analysis = _protocol({"field_model": "pulsed"}).calc_solution(target, _array(), simulate=True, scale=True)
    res = sol.simulation_result
    pmax, pmin, inten = (np.array(res[k].data) for k in ("p_max", "p_min", "intensity"))
    assert not np.array_equal(pmax, pmin)
    # the scaled mainlobe p_min peak is the target pressure, per focus
    assert np.allclose(analysis.mainlobe_pnp_MPa, 1.0, rtol=1e-5)
    # aggregate: max over foci of the scaled per-focus volumes, p_max on its own
    assert np.array_equal(np.asarray(agg["p_max"].data), pmax.max(axis=0))
    assert np.array_equal(np.asarray(agg["p_min"].data), pmin.max(axis=0))
    # the analysis again, from the host volumes (uploaded: no p_max on the device) -- the same report
    again = sol.analyze()
    for name in ("mainlobe_pnp_MPa", "mainlobe_isppa_Wcm2", "sidelobe_pnp_MPa", "global_pnp_MPa", "global_isppa_Wcm2",
                 "beamwidth_lat_3dB_mm", "focal_centroid_ax_mm"):
        assert np.allclose(getattr(again, name), getattr(analysis, name), rtol=1e-6, equal_nan=True), name
    assert np.allclose(np.asarray(sol.get_ita().data), 1e3 * inten * sol.get_pulsetrain_dutycycle() * sol.get_sequence_dutycycle(), rtol=1e-5)
    # file round trip keeps the two volumes apart
    sol.to_files(tmp_path / "sol.json")
    back = ol.Solution.from_files(tmp_path / "sol.json")
    assert np.array_equal(np.asarray(back.simulation_result["p_max"].data), pmax)
    assert np.array_equal(np.asarray(back.simulation_result["p_min"].data), pmin)


@pytest.mark.gpu
def test_calc_solution_cw_option_is_the_default():
    target = ol.Point(position=(0, 0, 30), units="mm")
    outs = []
    for opts in ({}, {"field_model": "cw"}):
        sol, agg, analysis = _protocol(opts).calc_solution(target, _array(), simulate=True, scale=True)
        outs.append(([np.array(sol.simulation_result[k].data) for k in ("p_max", "p_min", "intensity")] +
                     [np.array(agg[k].data) for k in ("p_max", "p_min", "intensity")], analysis))
    for a, b in zip(outs[0][0], outs[1][0]):
        assert np.array_equal(a, b)
    assert np.array_equal(outs[0][0][0], outs[0][0][1])          # CW: p_max == p_min
    # the report: the centroids are fp64 sums accumulated atomically (olx_field_masked_moments), equal to rounding from run to run
    for fld in dataclasses.fields(outs[0][1]):
        a, b = getattr(outs[0][1], fld.name), getattr(outs[1][1], fld.name)
        if isinstance(a, (list, float)):
            assert np.allclose(np.asarray(a, dtype=float), np.asarray(b, dtype=float), rtol=1e-12, atol=1e-12, equal_nan=True), fld.name
        else:
            assert a == b, fld.name


@pytest.mark.gpu
def test_run_simulation_pulsed_schema():
    arr = _array()
    setup = ol.SimSetup(spacing=1.0, x_extent=(-10, 10), y_extent=(-10, 10), z_extent=(5, 35))
    params = setup.setup_sim_scene(ol.seg.seg_methods.UniformWater())
    ds_, raw = sf.run_simulation(arr, params, freq=F0, cycles=6, dt=0, t_end=0, cfl=0.5, amplitude=1, field_model="pulsed")
    assert np.array_equal(raw["p_max"], np.asarray(ds_["p_max"].data)) and np.array_equal(raw["p_min"], -np.asarray(ds_["p_min"].data))
    assert not np.array_equal(np.asarray(ds_["p_max"].data), np.asarray(ds_["p_min"].data))
    with pytest.raises(NotImplementedError, match="directivity"):
        sf.run_simulation(arr, params, freq=F0, field_model="pulsed", directivity=True)


# ---- 15. the debug library ----------------------------------------------------------------------------------------------------------
def test_pulse_bounds_tag_only_in_the_debug_library():
    prod = open(os.path.join(LIB, "libolx.so"), "rb").read()
    dbg = open(os.path.join(LIB, "libolx_dbg.so"), "rb").read()
    assert b"olx_dbg_bounds_pulse" in dbg and b"olx_dbg_bounds_pulse" not in prod


@pytest.mark.gpu
def test_pulsed_kernels_stay_inside_their_extents_in_the_debug_library():
    env = dict(os.environ, OLX_LIB_PATH=os.path.join(LIB, "libolx_dbg.so"))
    sel = "matches_oracle_small or window_longer or late_arrivals or half_step"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", sel, "-p", "no:cacheprovider"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=1200)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in tail and "failed" not in tail, tail
