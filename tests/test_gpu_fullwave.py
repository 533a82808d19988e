"""Full-wave model on the MI355X: kernel 5 (fullwave_*_k) through the C-ABI against the fp64 oracle of the same discrete scheme
(tests/fullwave_oracle.py) over the case table of tests/fullwave_cases.py -- full volumes of p_max, p_min and sum p^2, and the traces
-- then run_fullwave_simulation end to end, as the seam of Protocol.calc_solution, in the debug library, and next to the other resident
objects of the context.

Gate: the largest deviation measured over the case table, as a fraction of each record's maximum, was
2.17e-6 (the trace of the lossless case; p_max / p_min <= 6.4e-7, sum p^2 <= 1.5e-6); the gate is eight times that, rounded up to one
digit: 2e-5.  The margin covers fused-multiply-add and ordering differences across compiler versions."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import openlifu_amd as ol
from openlifu_amd import _native as nat
from openlifu_amd.plan import protocol as protocol_module
from openlifu_amd.seg.material import Material
from openlifu_amd.seg.seg_methods.threshold import SkullThreshold, skull_slab_image
from openlifu_amd.sim import run_fullwave_simulation, run_thermal_simulation
from openlifu_amd.util import dataset as ds
import fullwave_cases as fc
import fullwave_oracle as fo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "openlifu-python_amd", "lib")
GATE = 2e-5
FREQ = 500e3


@pytest.fixture(scope="module")
def ctx():
    c = nat.Context(0)
    yield c
    c.close()


def check_gate(got, ref):
    dev = fc.deviations(got, ref)
    print({k: f"{v:.3e}" for k, v in dev.items()})
    for key, v in dev.items():
        assert v <= GATE, (key, v)


# ---- parity with the oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_matches_oracle(ctx, name):
    k = fc.CASES[name]
    # the oracle and the device take the same activity decisions: no burst edge within 1e-6 of a step's injection time
    assert fo.activity_margin(k["tau"], k["cycles"] / k["freq"], k["dt"]) >= 1e-6
    assert 200 <= k["steps"] <= 600
    got = fc.run_device(ctx, name)
    ref = fc.reference(name)
    assert ref["p_max"].max() > 0 and ref["p_min"].max() > 0
    check_gate(got, ref)
    assert got[0].min() >= 0 and got[1].min() >= 0          # both records start from 0


@pytest.mark.gpu
def test_continued_run_equals_one_shot_bit_for_bit(ctx):
    one = fc.run_device(ctx, "layered")
    two = fc.run_device(ctx, "layered", split=137)
    for a, b in zip(one, two):
        assert np.array_equal(a, b)
    # ... and a run is reproducible (no atomics, no race between the entries of a shared voxel)
    for a, b in zip(one, fc.run_device(ctx, "layered")):
        assert np.array_equal(a, b)


@pytest.mark.gpu
def test_smaller_plan_after_a_larger_one(ctx):
    fc.run_device(ctx, "layered")
    check_gate(fc.run_device(ctx, "short_axis"), fc.reference("short_axis"))
    check_gate(fc.run_device(ctx, "uniform_water"), fc.reference("uniform_water"))


@pytest.mark.gpu
def test_sum_of_squares_is_opt_in(ctx):
    with_sq = fc.run_device(ctx, "uniform_water", psq=True)
    without = fc.run_device(ctx, "uniform_water", psq=False)
    assert without[2] is None
    for a, b in ((with_sq[0], without[0]), (with_sq[1], without[1]), (with_sq[3], without[3])):
        assert np.array_equal(a, b)
    with pytest.raises(nat.NativeError, match="did not accumulate"):
        ctx._fw_psq = True
        ctx.fullwave_fetch()


@pytest.mark.gpu
def test_calls_out_of_order_and_bad_arguments():
    c = nat.Context(0)
    try:
        with pytest.raises(nat.NativeError, match="no full-wave plan"):
            c.fullwave_sources([0], [1.0], [0.0], FREQ, 3, 0, 10)
        k = fc.CASES["uniform_water"]
        with pytest.raises(ValueError, match="stability bound"):
            c.fullwave_plan(k["h"], k["n"], 1500.0, 1000.0, 0.0, 1500.0, 6, 2.0, 2 * fc.bound(k["h"], 1500.0))
        bad = np.full(k["n"], 1500.0, dtype=np.float32); bad[3, 4, 5] = np.nan
        with pytest.raises(ValueError, match="sound speed"):
            c.fullwave_plan(k["h"], k["n"], bad, 1000.0, 0.0, 1500.0, 6, 2.0, k["dt"])
        with pytest.raises(ValueError, match="scalars of NULL volumes"):
            c.fullwave_plan(k["h"], k["n"], 1500.0, -1.0, 0.0, 1500.0, 6, 2.0, k["dt"])
        with pytest.raises(ValueError, match="no interior"):
            c.fullwave_plan(k["h"], (5, 21, 23), 1500.0, 1000.0, 0.0, 1500.0, 3, 2.0, k["dt"])
        assert c.fullwave_plan(k["h"], k["n"], 1500.0, 1000.0, 0.0, 1500.0, 6, 2.0, k["dt"]) == pytest.approx(fc.bound(k["h"], 1500.0), rel=1e-12)
        c._fw_steps = 10
        with pytest.raises(nat.NativeError, match="olx_fullwave_sources first"):
            c.fullwave_run(0, 10)
        with pytest.raises(ValueError, match="outside the grid"):
            c.fullwave_sources([int(np.prod(k["n"]))], [1.0], [0.0], FREQ, 3, 0, 10)
        c.fullwave_sources([5], [1.0], [0.0], FREQ, 3, 0, 10)
        c._fw_ran, c._fw_psq = 0, False
        with pytest.raises(nat.NativeError, match="nothing run"):
            c.fullwave_fetch()
        with pytest.raises(nat.NativeError, match="does not continue"):
            c.fullwave_run(4, 2)
        with pytest.raises(ValueError, match="outside the run"):
            c.fullwave_run(0, 11)
        c.fullwave_run(0, 4)
        with pytest.raises(nat.NativeError, match="keeps the accumulation"):
            c.fullwave_run(4, 2, psq=True)
        c.fullwave_run(4, 6)
        c.sync()
    finally:
        c.close()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
MATS = {"water": Material("water", 1500.0, 1000.0, 0.0, 4182.0, 0.598), "skull": Material("skull", 2800.0, 1900.0, 6.0, 1300.0, 0.4)}
PML = 6


def _setup():
    return ol.SimSetup(spacing=0.5, x_extent=(-6, 6), y_extent=(-6, 6), z_extent=(0, 16))


def _array():
    return ol.Transducer.gen_matrix_array(nx=4, ny=4, pitch=2.1, kerf=0.2, units="mm", sensitivity=1e5)


def _volume(setup):
    coords = setup.get_coords()
    xs, ys, zs = (np.asarray(c.data) * 1e-3 for c in coords.values())
    dims = list(coords.keys() if not hasattr(coords, "dims") else coords.dims)
    return ds.make_dataarray(skull_slab_image(xs, ys, zs), coords=coords, dims=dims, name="ct")


def _focus_delays(arr, focus_m, c=1500.0):
    pos = arr.element_table()[0]
    d = np.sqrt(((pos - np.asarray(focus_m)) ** 2).sum(axis=1))
    return (d.max() - d) / c + 0.37e-7        # (off the injection times)


def _oracle_for(arr, params, delays, apod, cycles, amplitude, ramp, trace_ijk):
    """The oracle fed with inputs formed here, from the definition: padded volumes, source entries, time axis."""
    xs, ys, zs = (np.asarray(params.coords[d].data, dtype=np.float64) * 1e-3 for d in ("x", "y", "z"))
    h = np.array([xs[1] - xs[0], ys[1] - ys[0], zs[1] - zs[0]])
    n = (xs.size, ys.size, zs.size)
    c = np.asarray(params["sound_speed"].data, dtype=np.float64)
    rho = np.asarray(params["density"].data, dtype=np.float64)
    alpha = np.asarray(params["attenuation"].data, dtype=np.float64) * (FREQ * 1e-6) ** 0.9 * 100.0 / 8.685889638065035
    dt_max = 6.0 / (7.0 * c.max() * np.sqrt(np.sum(1.0 / h ** 2)))
    dt = min(0.3 * h.min() / c.max(), 0.9 * dt_max)
    t_end = np.sqrt(np.sum((np.array(n) * h) ** 2)) / c.min() + delays.max() + cycles / FREQ
    steps = int(np.ceil(t_end / dt))
    pos, _, area, _, _ = arr.element_table()
    A = apod * area * amplitude * float(arr.sensitivity) * FREQ / 1500.0
    cp, rp, ap = (np.pad(v, PML, mode="edge") for v in (c, rho, alpha))
    npad = tuple(v + 2 * PML for v in n)
    origin = np.array([xs[0], ys[0], zs[0]]) - PML * h
    ijk, amp, tau = fo.monopole_entries(pos, origin, h, A, delays, cp, FREQ, dt, npad)
    assert fo.activity_margin(tau, cycles / FREQ, dt) >= 1e-6
    ref = fo.simulate(npad, h, cp, rp, ap, 1500.0, PML, 2.0, dt, steps, ijk, amp, tau, FREQ, cycles, ramp, trace_ijk=np.asarray(trace_ijk) + PML)
    crop = (slice(PML, -PML),) * 3
    return {k: (v[crop] if v.ndim == 3 else v) for k, v in ref.items()}, dt, steps, c, rho


@pytest.mark.gpu
@pytest.mark.parametrize("medium", ["water", "skull"])
def test_run_fullwave_simulation_end_to_end(medium):
    arr, setup = _array(), _setup()
    params = setup.setup_sim_scene(SkullThreshold(materials=MATS), volume=_volume(setup)) if medium == "skull" else setup.setup_sim_scene(ol.seg_methods.UniformWater())
    delays = _focus_delays(arr, (0.0, 0.0, 12e-3))
    apod = np.ones(16); apod[5] = 0.0; apod[9] = 0.5
    pts = [[0.0, 0.0, 12.0], [1.2, -2.2, 6.1]]
    out, raw = run_fullwave_simulation(arr, params, delays, apod, freq=FREQ, cycles=3, amplitude=2.0, pml_size=PML, ramp_cycles=1.0,
                                       pulse_intensity_integral=True, record_points=pts)
    tr_ijk = np.array([[12, 12, 24], [14, 8, 12]])
    ref, dt, steps, c, rho = _oracle_for(arr, params, delays, apod, 3.0, 2.0, 1.0, tr_ijk)
    assert raw["dt"] == pytest.approx(dt, rel=1e-14) and raw["n_steps"] == steps and 200 <= steps <= 600
    assert raw["backend"] == "openlifu_amd/hip-gfx950" and raw["points_per_wavelength"] == pytest.approx(1500.0 / (FREQ * 0.5e-3))
    assert {"p_max", "p_min", "dt", "n_steps", "points_per_wavelength", "backend", "p_trace", "t", "trace_voxels"} <= set(raw)
    n = ref["p_max"].shape
    assert list(raw["trace_voxels"]) == [int((i * n[1] + j) * n[2] + k) for i, j, k in tr_ijk]
    assert raw["p_trace"].shape == (2, steps) and np.allclose(raw["t"], (np.arange(steps) + 1) * dt, rtol=1e-14, atol=0)
    if medium == "skull":
        assert c.max() == 2800.0 and c.min() == 1500.0
    pmax, pmin = np.asarray(out["p_max"].data), np.asarray(out["p_min"].data)
    assert pmax.shape == n and pmax.dtype == np.float32 and out["p_min"].attrs["units"] == "Pa"
    assert np.abs(pmax - ref["p_max"]).max() <= GATE * ref["p_max"].max()
    assert np.abs(pmin - ref["p_min"]).max() <= GATE * ref["p_min"].max()
    assert np.array_equal(raw["p_max"], pmax) and np.array_equal(raw["p_min"], -pmin)
    assert np.abs(raw["p_trace"].T - ref["trace"]).max() <= GATE * np.abs(ref["trace"]).max()
    # intensity and PII with the voxel's own rho c
    inten = 1e-4 * ref["p_min"] ** 2 / (2 * rho * c)
    assert out["intensity"].attrs["units"] == "W/cm^2"
    assert np.abs(np.asarray(out["intensity"].data) - inten).max() <= 4 * GATE * inten.max()
    pii = 1e-4 * dt * ref["psq"] / (rho * c)
    assert out["pulse_intensity_integral"].attrs["units"] == "J/cm^2"
    assert np.abs(np.asarray(out["pulse_intensity_integral"].data) - pii).max() <= GATE * pii.max()
    assert pmin[12, 12, 24] > 0 and pmax[12, 12, 24] > 0          # the wave reached the focus


@pytest.mark.gpu
def test_as_the_seam_of_calc_solution(monkeypatch):
    arr, setup = _array(), _setup()
    proto = ol.Protocol(pulse=ol.Pulse(frequency=FREQ, duration=6e-6), sequence=ol.Sequence(pulse_count=2, pulse_train_interval=0),
                        focal_pattern=ol.focal_patterns.Wheel(center=False, num_spokes=2, spoke_radius=1.5, target_pressure=1e6),
                        sim_setup=setup, seg_method=SkullThreshold(materials=MATS), apod_method=ol.apod_methods.Uniform())
    seam = functools.partial(run_fullwave_simulation, pml_size=PML)
    monkeypatch.setattr(protocol_module, "run_simulation", seam)
    vol = _volume(setup)
    target = ol.Point(position=(0, 0, 12), units="mm")
    sol, agg, analysis = proto.calc_solution(target, arr, volume=vol, simulate=True, scale=False)
    assert analysis is not None and len(sol.foci) == 2
    params = setup.setup_sim_scene(proto.seg_method, volume=vol)
    for i in range(2):
        direct, _ = seam(arr=arr, params=params, delays=sol.delays[i], apod=sol.apodizations[i], freq=FREQ, cycles=3.0, dt=setup.dt,
                         t_end=setup.t_end, cfl=setup.cfl, amplitude=proto.pulse.amplitude)
        for key in ("p_max", "p_min", "intensity"):
            assert np.array_equal(np.asarray(sol.simulation_result[key].data)[i], np.asarray(direct[key].data)), (i, key)
    assert np.allclose(np.asarray(agg["p_min"].data), np.asarray(sol.simulation_result["p_min"].data).max(axis=0))
    assert not np.array_equal(np.asarray(sol.simulation_result["p_min"].data)[0], np.asarray(sol.simulation_result["p_min"].data)[1])


# ---- a full-wave run changes nothing else -------------------------------------------------------------------------------------------
def _plain(a):
    return repr(a.to_dict() if hasattr(a, "to_dict") else vars(a))


@pytest.mark.gpu
def test_full_wave_run_leaves_the_other_resident_objects_untouched():
    arr = ol.Transducer.gen_matrix_array(nx=4, ny=4, pitch=2.1, kerf=0.2, units="mm", sensitivity=1e5)
    setup = _setup()
    mats = {"water": Material("water", 1500.0, 1000.0, 0.0022, 4182.0, 0.598), "skull": Material("skull", 2800.0, 1900.0, 6.0, 1300.0, 0.4)}
    proto = ol.Protocol(pulse=ol.Pulse(frequency=FREQ, duration=2e-5), sequence=ol.Sequence(pulse_interval=0.1, pulse_count=2, pulse_train_interval=1.0, pulse_train_count=1),
                        focal_pattern=ol.focal_patterns.Wheel(center=False, num_spokes=2, spoke_radius=1.5, target_pressure=1e6),
                        sim_setup=setup, seg_method=SkullThreshold(materials=mats), apod_method=ol.apod_methods.Uniform())
    vol = _volume(setup)
    sol, _, _ = proto.calc_solution(ol.Point(position=(0, 0, 12), units="mm"), arr, volume=vol, simulate=True, scale=True)
    params = setup.setup_sim_scene(proto.seg_method, volume=vol)
    run_thermal_simulation(params, sol)
    eng = ol.get_engine()
    assert sol._device_is_current()
    variant = eng.ctx.field_variant()
    before = (eng.ctx.field_fetch_all(), eng.ctx.thermal_fetch(), _plain(sol.analyze()))
    run_fullwave_simulation(arr, params, sol.delays[0], sol.apodizations[0], freq=FREQ, cycles=3, pml_size=PML, pulse_intensity_integral=True,
                            record_points=[[0.0, 0.0, 12.0]])
    assert sol._device_is_current() and eng.ctx.field_variant() == variant
    after = (eng.ctx.field_fetch_all(), eng.ctx.thermal_fetch(), _plain(sol.analyze()))
    for key in ("pmag", "intensity"):
        assert np.array_equal(before[0][key], after[0][key]), key
    for a, b in zip(before[1], after[1]):
        assert np.array_equal(a, b)
    assert before[2] == after[2]
    eng.ctx.field_launch()          # the plan still launches, to the same bits (the solution was scaled: compare unscaled launches)
    again = eng.ctx.field_fetch_all()
    eng.ctx.field_launch()
    assert np.array_equal(again["pmag"], eng.ctx.field_fetch_all()["pmag"])


# ---- the debug library --------------------------------------------------------------------------------------------------------------
def test_fullwave_bounds_tag_only_in_the_debug_library():
    prod = open(os.path.join(LIB, "libolx.so"), "rb").read()
    dbg = open(os.path.join(LIB, "libolx_dbg.so"), "rb").read()
    assert b"olx_dbg_bounds_fullwave" in dbg and b"olx_dbg_bounds_fullwave" not in prod


@pytest.mark.gpu
def test_fullwave_kernels_stay_inside_their_extents_in_the_debug_library():
    env = dict(os.environ, OLX_LIB_PATH=os.path.join(LIB, "libolx_dbg.so"))
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "from openlifu_amd import _native as nat\n"
            "import fullwave_cases as fc\n"
            "ctx = nat.Context(0)\n"
            "for name in sorted(fc.CASES):\n"
            "    dev = fc.deviations(fc.run_device(ctx, name), fc.reference(name))\n"
            "    assert max(dev.values()) <= %r, (name, dev)\n"
            "fc.run_device(ctx, 'layered', split=137)\n"
            "ctx.sync()\n"
            "print('fullwave debug cases ok')\n") % (os.path.join(ROOT, "tests"), os.path.join(ROOT, "openlifu-python_amd"), GATE)
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "fullwave debug cases ok" in tail, tail
