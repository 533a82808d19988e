"""The pulse intensity integral through the C-ABI (olx_pii_post and its neighbours), Protocol.calc_solution and Solution on the MI355X,
against the fp64 oracle tests/pii_solution_oracle.py (whose scenes these tests use; their mask margins are asserted in
tests/test_pii_solution_host.py).  Exactness contracts (DESIGN.md section 2 "pulse energy"): the scaled volumes, max_f PII_f and every peak
are bit-equal to their fp32 definitions; the weighted volume lies within (2 F + 4) 2^-24 of the oracle's volume maximum -- one rounding per
fma, one per weight, one for g_f and one for the scaled product."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import openlifu_amd as ol
from openlifu_amd import _native as nat
from openlifu_amd.plan.solution import PII
from openlifu_amd.sim import field as sf
from openlifu_amd.sim import run_thermal_simulation
from openlifu_amd.util import dataset as ds
from oracle import bf_oracle as bo
from conftest import synthetic_array
import pii_solution_oracle as pso

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "openlifu-python_amd", "lib")
F0, C, RHO, P0, CYCLES = 400e3, 1500.0, 1000.0, 1e5, 6
EPS = 2.0 ** -24


def weighted_gate(F):
    return (2 * F + 4) * EPS


def plan_pulsed(ctx, F, n, pii=True):
    """8 x 8 array at 2 mm pitch, 6 cycles at 400 kHz, the oracle's steering to pso.FOCI_MM[F]: planned, not launched."""
    pos_mm, _, size = synthetic_array(8, 8, 2.0)
    pos_m = pos_mm * 1e-3
    ctx.set_elements(pos_m, np.tile([0.0, 0.0, 1.0], (len(pos_m), 1)), size[:, 0] * size[:, 1] * 1e-6)
    steer = [bo.beamform(pos_m, np.zeros_like(pos_m), f, C) for f in np.asarray(pso.FOCI_MM[F]) * 1e-3]
    ctx.set_steering(np.array([s[0] for s in steer]), np.array([s[1] for s in steer]))
    xs, ys, zs = pso.grid_axes(n)
    sp = [xs[1] - xs[0], ys[1] - ys[0], zs[1] - zs[0]]
    dt, n_t = sf.pulse_time_axis(sp, n, 0.0, 0.0, 0.5)
    ctx.field_pulse(CYCLES, dt, n_t)
    try:
        ctx.field_plan((xs[0], ys[0], zs[0]), sp, n, F0, C, RHO, P0, flags=nat.OUT_PMAG | nat.OUT_INTENSITY | nat.OUT_PMAX | (nat.OUT_PII if pii else 0))
    finally:
        ctx.field_pulse(0.0, 0.0, 0)
    return xs, ys, zs


# ---- 1. olx_pii_post through the ctypes context ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("grid", sorted(pso.GRIDS))
@pytest.mark.parametrize("F", [1, 3, 8])
def test_pii_post_every_form(ctx, F, grid):
    n = pso.GRIDS[grid]
    xs, ys, zs = plan_pulsed(ctx, F, n)
    ctx.field_launch()
    raw = ctx.pii_fetch(F)
    assert raw.shape == (F,) + n and raw.dtype == np.float32 and raw.min() >= 0 and all(raw[f].max() > 0 for f in range(F))
    s = np.linspace(0.37, 1.93, F) if F > 1 else np.array([1.37])
    w = pso.pulses_per_focus(10, F) / pso.sequence_period(0.1, 10, 0.0)
    A = pso.frames_for(pso.FOCI_MM[F])
    msk = pso.masks(A, pso.ASPECT, xs, ys, zs, pso.R_MAIN, pso.R_SIDE, pso.ZMIN)
    mask_args = dict(A=A, aspect=pso.ASPECT, r_main_m=pso.R_MAIN, r_side_m=pso.R_SIDE, zmin_m=pso.ZMIN)
    for k, (use_s, use_w, use_a) in enumerate(itertools.product((False, True), repeat=3)):
        label = f"F={F} {grid} scale={use_s} weights={use_w} frames={use_a}"
        if k > 0:
            ctx.pii_upload(raw)            # (the first form works on the launched volumes, the others on the same values uploaded again)
        kw = dict(weights=w if use_w else None, **(mask_args if use_a else {}))
        got = ctx.pii_post(F, scale=s if use_s else None, **kw)
        want = pso.scaled(raw, s) if use_s else raw
        vols = ctx.pii_fetch(F)
        assert np.array_equal(vols, want), label
        vmax = ctx.pii_fetch_max()
        assert np.array_equal(vmax, pso.pii_max(vols)), label
        wvol = None
        if use_w:
            wvol = ctx.pii_fetch_weighted()
            ref = pso.weighted(pso.scaled(raw, s) if use_s else raw, w)
            err = np.abs(wvol.astype(np.float64) - ref).max() / ref.max()
            print(f"[pii_post] {label}: weighted volume {err / EPS:.2f} x 2^-24 of its maximum (gate {2 * F + 4})")
            assert err <= weighted_gate(F), label
        else:
            with pytest.raises(nat.NativeError, match="olx_pii_fetch_weighted"):
                ctx.pii_fetch_weighted()
        if use_a:
            pk, glob = got
            ref_pk, ref_glob = pso.peaks(vols, wvol, msk)
            assert np.array_equal(pk, ref_pk) and np.float32(glob) == ref_glob, (label, pk, ref_pk, glob, ref_glob)
            assert np.all(pk[:, 0] > 0) and np.all(pk[:, 2] >= pk[:, 1])
        else:
            assert got is None
        # the same call without factors: nothing moves
        again = ctx.pii_post(F, scale=None, **kw)
        assert np.array_equal(ctx.pii_fetch(F), vols) and np.array_equal(ctx.pii_fetch_max(), vmax), label
        if use_w:
            assert np.array_equal(ctx.pii_fetch_weighted(), wvol), label
        if use_a:
            assert np.array_equal(again[0], got[0]) and again[1] == got[1], label
    ctx.sync()


# ---- the Solution scene -----------------------------------------------------------------------------------------------------------------
def solve(pii=True, scale=True, pulse_count=9):
    proto = pso.solution_protocol(pii=pii, pulse_count=pulse_count)
    sol, agg, an = proto.calc_solution(ol.Point(position=pso.SOLUTION_TARGET_MM, units="mm"), pso.solution_array(), simulate=True, scale=scale)
    return proto, sol, agg, an


def solution_grid_m(sol):
    return tuple(np.asarray(sol.simulation_result.coords[d].data) * 1e-3 for d in ("x", "y", "z"))


def oracle_masks(sol, opts):
    return pso.masks(sol._focus_frames(), opts.mainlobe_aspect_ratio, *solution_grid_m(sol), opts.mainlobe_radius, opts.sidelobe_radius,
                     opts.sidelobe_zmin)


def expected_analysis(sol, opts, pii32):
    """PulseEnergyAnalysis numbers from the oracle's masks on the float32 volumes given (and the device's weighted volume of them)."""
    n_f, period, length = pso.pulses_per_focus(sol.sequence.pulse_count, sol.num_foci()), sol.sequence_period(), sol.pulse_length()
    return n_f, period, length, oracle_masks(sol, opts)


# ---- 2. calc_solution end to end ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_calc_solution_carries_the_scaled_pii():
    proto, sol, agg, _ = solve(pii=True, scale=True)
    res = sol.simulation_result
    da = res[PII]
    assert isinstance(da, ds.LazyDataArray) and not da.materialized
    assert tuple(da.shape) == (3, 17, 17, 25) and tuple(da.dims) == ("focal_point_index", "x", "y", "z")
    assert da.attrs["units"] == "J/cm^2" and da.attrs["long_name"]
    assert isinstance(agg[PII], ds.LazyDataArray) and agg[PII].attrs["units"] == "J/cm^2" and tuple(agg[PII].shape) == (17, 17, 25)
    # the option-off call: today's variables, and the same pressures and intensity bit for bit
    _, sol0, agg0, _ = solve(pii=False, scale=True)
    assert sorted(sol0.simulation_result.data_vars) == ["intensity", "p_max", "p_min"] and sorted(agg0.data_vars) == ["intensity", "p_max", "p_min"]
    assert sorted(res.data_vars) == ["intensity", "p_max", "p_min", PII] and sorted(agg.data_vars) == ["intensity", "p_max", "p_min", PII]
    assert sorted(solve(pii=None, scale=False)[1].simulation_result.data_vars) == ["intensity", "p_max", "p_min"]
    want0 = {k: np.asarray(sol0.simulation_result[k].data) for k in ("p_min", "p_max", "intensity")}
    agg_want0 = {k: np.asarray(agg0[k].data) for k in ("p_min", "p_max", "intensity")}
    proto, sol, agg, _ = solve(pii=True, scale=True)          # (the option-off call took the device: run the option-on call again)
    res = sol.simulation_result
    got = np.asarray(res[PII].data)
    assert got.dtype == np.float32 and not res["p_min"].materialized
    for k in want0:
        assert np.array_equal(np.asarray(res[k].data), want0[k]), k
        assert np.array_equal(np.asarray(agg[k].data), agg_want0[k]), k
    assert np.array_equal(np.asarray(agg[PII].data), got.max(axis=0))
    # the unscaled PII of every focus from run_simulation on the same scene, times float32(s_f^2): uniform apodization and voltage 1, so
    # the factor Solution.scale applied to the pressures of focus f is exactly voltage * apodization
    s = sol.voltage * sol.apodizations.max(axis=1)
    assert np.all(sol.apodizations == sol.apodizations[:, :1]) and np.ptp(s) > 0
    params = proto.sim_setup.setup_sim_scene(proto.seg_method)
    arr = pso.solution_array()
    raw = np.stack([np.asarray(sf.run_simulation(arr, params, delays=sol.delays[f], apod=np.ones(arr.numelements()), freq=F0, cycles=CYCLES,
                                                 dt=0, t_end=0, cfl=0.5, amplitude=proto.pulse.amplitude, field_model="pulsed",
                                                 pulse_intensity_integral=True)[0][PII].data) for f in range(3)])
    assert np.array_equal(got, pso.scaled(raw, s))
    # scale=False: the unscaled volumes themselves, and their maximum
    _, sol_u, agg_u, _ = solve(pii=True, scale=False)
    assert np.array_equal(np.asarray(sol_u.simulation_result[PII].data), raw)
    assert np.array_equal(np.asarray(agg_u[PII].data), raw.max(axis=0))


@pytest.mark.gpu
def test_solution_scale_scales_the_pii_once_on_the_device_and_on_the_host():
    _, host, _, _ = solve(pii=True, scale=False)
    raw = np.asarray(host.simulation_result[PII].data).copy()          # (host: read to the host here; sol below stays on the device)
    proto, sol, _, _ = solve(pii=True, scale=False)
    assert sol._pii_on_device() and not host._pii_on_device()
    v0 = sol.voltage
    sol.scale(proto.focal_pattern, analysis_options=proto.analysis_options)
    s = sol.voltage / v0 * sol.apodizations.max(axis=1)
    dev = np.asarray(sol.simulation_result[PII].data)
    assert np.array_equal(dev, pso.scaled(raw, s))
    host.scale(proto.focal_pattern, analysis_options=proto.analysis_options)
    assert np.array_equal(np.asarray(host.simulation_result[PII].data), dev)


# ---- 3. analyze_pulse_energy -------------------------------------------------------------------------------------------------------------
def check_analysis(an, sol, opts, pii32):
    F = sol.num_foci()
    n_f, period, length, msk = expected_analysis(sol, opts, pii32)
    assert an.pulses_per_focus == n_f.tolist() and an.pulse_length_s == length == CYCLES / F0 and an.sequence_period_s == period
    ref_ta = pso.weighted(pii32, n_f / period)
    pk, _ = pso.peaks(pii32, None, msk)
    for f in range(F):
        assert an.mainlobe_pii_mJcm2[f] == float(pk[f, 0]) * 1e3 and an.sidelobe_pii_mJcm2[f] == float(pk[f, 1]) * 1e3
        assert an.global_pii_mJcm2[f] == float(pk[f, 2]) * 1e3 and pk[f, 0] > 0
        assert abs(an.mainlobe_isppa_Wcm2[f] - float(pk[f, 0]) / length) <= 1e-12 * float(pk[f, 0]) / length
        # I_spta: the peak of the device's fp32 weighted volume, within the derived bound of the fp64 volume's peak under the same mask
        want = ref_ta[msk[0][f]].max() * 1e3
        assert abs(an.mainlobe_ispta_mWcm2[f] - want) <= weighted_gate(F) * ref_ta.max() * 1e3, f
    assert abs(an.global_ispta_mWcm2 - ref_ta[msk[2]].max() * 1e3) <= weighted_gate(F) * ref_ta.max() * 1e3


@pytest.mark.gpu
def test_analyze_pulse_energy_on_the_device_and_after_upload():
    proto, sol, _, _ = solve(pii=True, scale=True)
    opts = proto.analysis_options
    assert sol._pii_on_device()
    an = sol.analyze_pulse_energy(opts)
    assert sol._pii_on_device() and not sol.simulation_result[PII].materialized          # nothing crossed to the host
    # exact: the peaks against the device's own fetched volumes under the oracle's masks, the host divisions in fp64
    eng = ol.get_engine()
    n_f, period, length, msk = expected_analysis(sol, opts, None)
    wvol = eng.ctx.pii_fetch_weighted()
    pii32 = np.asarray(sol.simulation_result[PII].data)
    pk, glob = pso.peaks(pii32, wvol, msk)
    for f in range(3):
        assert an.mainlobe_ispta_mWcm2[f] == float(pk[f, 3]) * 1e3
        assert abs(an.mainlobe_isppa_Wcm2[f] - float(pk[f, 0]) / (CYCLES / F0)) <= 1e-12 * an.mainlobe_isppa_Wcm2[f]
    assert an.global_ispta_mWcm2 == float(glob) * 1e3
    check_analysis(an, sol, opts, pii32)
    # the variable is on the host now; another launch takes the device: the next analysis uploads (olx_pii_upload) and agrees
    solve(pii=False, scale=False)
    assert not sol._pii_on_device()
    assert sol.analyze_pulse_energy(opts) == an


# ---- 4. get_pulse_dose -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_get_pulse_dose_uneven_counts():
    proto, sol, _, _ = solve(pii=True, scale=True)
    sol.sequence = ol.Sequence(pulse_interval=0.1, pulse_count=10, pulse_train_interval=1.0, pulse_train_count=1)
    assert sol.pulses_per_focus().tolist() == [3, 3, 4]
    dose = sol.get_pulse_dose()
    assert tuple(dose.dims) == ("x", "y", "z") and dose.attrs["units"] == "J/cm^2"
    got = np.asarray(dose.data)
    assert got.dtype == np.float32 and got.shape == (17, 17, 25)
    ref = pso.weighted(np.asarray(sol.simulation_result[PII].data), [3, 3, 4])
    err = np.abs(got.astype(np.float64) - ref).max() / ref.max()
    print(f"[dose] F=3, n_f=[3, 3, 4]: {err / EPS:.2f} x 2^-24 of the volume maximum (gate {2 * 3 + 4})")
    assert err <= weighted_gate(3)
    assert np.allclose(np.asarray(sol.get_pulse_dose(units="mJ/cm^2").data), got * 1e3, rtol=1e-6)      # (host path: the variable was read)
    assert np.allclose(np.asarray(sol.get_pulse_dose(units="J/m^2").data), got * 1e4, rtol=1e-6)
    for bad in ("W/cm^2", "J", "J/s", "xJ/cm^2"):
        with pytest.raises(ValueError, match="energy per area"):
            sol.get_pulse_dose(units=bad)


# ---- 5. thermal --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_thermal_heats_from_the_solutions_pii():
    proto, sol, _, _ = solve(pii=True, scale=True)
    params = proto.sim_setup.setup_sim_scene(proto.seg_method)
    res_ds, res_raw = run_thermal_simulation(params, sol, pulse_energy="solution")
    assert res_raw["source"] == "pulse_energy_resident" and not sol.simulation_result[PII].materialized
    rise = np.asarray(res_ds["temperature_rise_max"].data)
    assert rise.max() > 0
    E = np.asarray(sol.simulation_result[PII].data)                    # the fetched, scaled array
    arr_ds, arr_raw = run_thermal_simulation(params, sol, pulse_energy=E)
    assert arr_raw["source"] == "pulse_energy"
    ref = np.asarray(arr_ds["temperature_rise_max"].data)
    err = np.abs(rise.astype(np.float64) - ref).max() / ref.max()
    print(f"[thermal] resident PII against the uploaded array: {err:.3e} of the maximum rise {ref.max():.3e} K")
    assert err <= 1e-6
    # the variable has been read: the host path, the array's run bit for bit
    host_ds, host_raw = run_thermal_simulation(params, sol, pulse_energy="solution")
    assert host_raw["source"] == "pulse_energy"
    assert np.array_equal(np.asarray(host_ds["temperature_rise_max"].data), ref)


# ---- 6. files ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_files_round_trip(tmp_path):
    proto, sol, _, _ = solve(pii=True, scale=True)
    an = sol.analyze_pulse_energy(proto.analysis_options)
    sol.to_files(tmp_path / "sol.json")
    back = ol.Solution.from_files(tmp_path / "sol.json")
    want = np.asarray(sol.simulation_result[PII].data)
    got = back.simulation_result[PII]
    assert np.array_equal(np.asarray(got.data), want) and np.asarray(got.data).dtype == np.float32 and got.attrs["units"] == "J/cm^2"
    assert back.analyze_pulse_energy(proto.analysis_options) == an
    again = ol.Solution.from_json(sol.to_json(include_simulation_data=True))
    assert np.array_equal(np.asarray(again.simulation_result[PII].data), want)
    assert PII in sol.to_dict(include_simulation_data=True)["simulation_result"]


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals(ctx):
    target, arr = ol.Point(position=pso.SOLUTION_TARGET_MM, units="mm"), pso.solution_array()
    with pytest.raises(ValueError, match=r"pulse_intensity_integral.*field_model"):
        pso.solution_protocol(pii=True, field_model="cw").calc_solution(target, arr, simulate=True, scale=False)
    many = pso.solution_protocol(pii=True, pulse_count=9)
    many.focal_pattern = ol.focal_patterns.Wheel(center=True, num_spokes=8, spoke_radius=2.0, target_pressure=1e6)
    token = ol.get_engine().result_token
    with pytest.raises(ValueError, match="at most 8 foci"):
        many.calc_solution(target, arr, simulate=True, scale=False)
    assert ol.get_engine().result_token == token                        # refused before anything was simulated
    proto, sol, _, _ = solve(pii=False, scale=False)
    params = proto.sim_setup.setup_sim_scene(proto.seg_method)
    for call in (sol.analyze_pulse_energy, sol.get_pulse_dose, lambda: run_thermal_simulation(params, sol, pulse_energy="solution")):
        with pytest.raises(ValueError, match="pulse_intensity_integral"):
            call()
    with pytest.raises(ValueError, match='"solution"'):
        run_thermal_simulation(params, sol, pulse_energy="resident")
    # the C-ABI: nothing resident (no plan; a pulsed plan without OLX_OUT_PII; a plan with it that has not been launched)
    for call in (lambda: ctx.pii_post(3), lambda: ctx.pii_upload(np.zeros((1, 2, 2, 2), np.float32))):
        with pytest.raises(nat.NativeError):
            call()
    n = pso.GRIDS["odd17x17x25"]
    plan_pulsed(ctx, 3, n, pii=False)
    ctx.field_launch()
    with pytest.raises(nat.NativeError, match="no resident pulse intensity integrals"):
        ctx.pii_post(3)
    plan_pulsed(ctx, 3, n, pii=True)
    with pytest.raises(nat.NativeError, match="no resident pulse intensity integrals"):
        ctx.pii_post(3)
    ctx.field_launch()
    ctx.pii_post(3)
    for F in (2, 4):
        with pytest.raises(ValueError, match=f"{F} foci given, the resident pulse intensity integrals have 3"):
            ctx.pii_post(F)
    with pytest.raises(nat.NativeError, match="olx_thermal_source_pii"):
        ctx.thermal_source_pii(3)                                       # (no thermal plan)
    xs, ys, zs = pso.grid_axes(n)
    ctx.thermal_plan((xs[0], ys[0], zs[0]), [1e-3] * 3, n, 1000.0, 4182.0, 0.598, 0.1)
    with pytest.raises(ValueError, match="2 foci given, the resident pulse intensity integrals have 3"):
        ctx.thermal_source_pii(2)
    ctx.thermal_source_pii(3)
    ctx.pii_upload(np.ones((9,) + n, np.float32))
    with pytest.raises(ValueError, match="at most 8"):
        ctx.pii_post(9)
    ctx.sync()


# ---- 8. the debug library ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_pii_post_stays_inside_its_extents_in_the_debug_library():
    env = dict(os.environ, OLX_LIB_PATH=os.path.join(LIB, "libolx_dbg.so"))
    sel = "pii_post_every_form or thermal_heats_from_the_solutions_pii"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", sel, "-p", "no:cacheprovider"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "7 passed" in tail and "failed" not in tail, tail
