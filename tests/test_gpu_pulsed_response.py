"""Impulse-response drive of the pulsed model on the MI355X: kernel 2p's RESP instantiations through the C-ABI (olx_field_pulse_response)
against the fp64 pair-sum oracle (tests/pulsed_response_oracle.py) on full volumes -- p_max, p_min, intensity, PII and traces of every case
of tests/pulsed_response_cases.py -- their invariants, the refusals, run_simulation / Protocol.calc_solution with the opt-in, and the case
table in the debug library.

Gates (eight times the largest deviation measured over the case table, rounded up to one digit; voxels whose
t_e / dt or (t_e + T) / dt lies within 1e-7 of an integer excluded, as in tests/test_gpu_pulsed.py).  Measured on one MI355X: p_max 9.1e-7 and
p_min 8.9e-7 of the volume maximum, PII 9.9e-7 of its maximum, traces 9.5e-7 of the largest sample, intensity 1.3e-7 relative -- so
P_TOL = PII_TOL = TRACE_TOL = 8e-6 and I_TOL = 2e-6, below kernel 2p's own 1e-5 / 4e-5."""
import os
import subprocess
import sys

import numpy as np
import pytest

import openlifu_amd as ol
from openlifu_amd import _native as nat
from openlifu_amd.sim import field as sf
from openlifu_amd.sim import run_thermal_simulation
import pulsed_oracle as po
import pulsed_response_cases as pc
import pulsed_response_oracle as pro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "openlifu-python_amd", "lib")
F0, C, RHO, P0 = pc.F0, pc.C, pc.RHO, pc.P0
# p_max / p_min: of the oracle's volume maximum; PII: of its maximum; traces: of the largest oracle sample of the traced voxels;
# intensity: relative to 1e-4 p_min^2 / (2 rho c) of the p_min the kernel stored
P_TOL, PII_TOL, TRACE_TOL, I_TOL = 8e-6, 8e-6, 8e-6, 2e-6
MARGIN = 1e-7
GPU_CASES = ["ring30", "ring30_absorbing", "ring30_whole", "classes_9x9", "two_tap", "longer_than_burst", "taps255", "taps256", "cut_ringdown",
             "two_pass"]


@pytest.fixture(scope="module")
def ctx():
    c = nat.Context(0)
    yield c
    c.close()


def deviations(name, out, tr, vox):
    """dict(p_max, p_min, pii, trace, intensity) of the case's largest deviations from the oracle over all foci (see the gates above)."""
    k = pc.case(name)
    dev = dict(p_max=0.0, p_min=0.0, pii=0.0, trace=0.0, intensity=0.0)
    for f in range(len(k.delays)):
        ref = k.oracle(f)
        ok = ref["margin"] >= MARGIN
        for key, gpu, o in (("p_max", out["pmax"][f], ref["pmax"]), ("p_min", out["pmag"][f], ref["pmin"]), ("pii", out["pii"][f], ref["pii"])):
            dev[key] = max(dev[key], np.abs(gpu.ravel().astype(np.float64) - o)[ok].max() / o.max())
        it = 1e-4 * out["pmag"][f].astype(np.float64) ** 2 / (2 * RHO * C)
        nz = it > 1e-12 * it.max()
        dev["intensity"] = max(dev["intensity"], (np.abs(out["intensity"][f] - it)[nz] / it[nz]).max())
        tok = ok[vox]
        dev["trace"] = max(dev["trace"], np.abs(tr[f].astype(np.float64) - ref["p"][vox])[tok].max() / np.abs(ref["p"][vox]).max())
    return dev


def check_trace_invariants(name, out, tr, vox):
    """Exact zeros outside [first arrival, last burst end + M_max - 1) and max / -min of a trace == the volumes at its voxel, bit for bit."""
    k = pc.case(name)
    m_max = max(len(t) for t in k.taps)
    tdt = k.cycles / (F0 * k.dt)
    for f in range(len(k.delays)):
        live = k.apod[f] != 0
        u, _ = po.arrival_steps(k.pts[vox], k.pos_m[live], k.delays[f][live], k.dt, C, k.dmin)
        first, last = np.ceil(u).min(1).astype(int), np.ceil(u + tdt).max(1).astype(int) + m_max - 1
        ok = k.oracle(f)["margin"][vox] >= MARGIN
        for i in np.flatnonzero(ok):
            assert np.all(tr[f, i, :min(first[i], k.n_t)] == 0.0), (name, f, i)
            assert np.all(tr[f, i, min(last[i], k.n_t):] == 0.0), (name, f, i)
        assert np.array_equal(np.maximum(tr[f].max(1), 0.0), out["pmax"][f].ravel()[vox]), (name, f)
        assert np.array_equal(np.maximum(-tr[f].min(1), 0.0), out["pmag"][f].ravel()[vox]), (name, f)


# ---- the kernel against the oracle, full volumes ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", GPU_CASES)
def test_response_kernel_matches_oracle(ctx, name):
    k = pc.case(name)
    vox = k.trace_voxels()
    assert set(k.focus_voxels()) <= set(vox)
    out, tr = pc.run_device(ctx, name, trace=vox)
    assert out["variant"].endswith(f"; response: {len(k.taps)} classes, {max(len(t) for t in k.taps)} taps"), out["variant"]
    dev = deviations(name, out, tr, vox)
    print(f"[response] {name}: " + ", ".join(f"{key} {val:.3e}" for key, val in dev.items()))
    assert dev["p_max"] <= P_TOL and dev["p_min"] <= P_TOL and dev["pii"] <= PII_TOL and dev["trace"] <= TRACE_TOL and dev["intensity"] <= I_TOL, dev
    check_trace_invariants(name, out, tr, vox)
    if name == "cut_ringdown":          # t_end falls inside the ring-down of the focus voxel: the last sample still rings
        assert np.all(np.abs(tr[:, list(vox).index(k.focus_voxels()[0]), -1]) > 0)
    if name == "two_pass":
        assert k.cycles / (F0 * k.dt) + 100 > 2 * (64 * 21 - 99)          # three passes of 1344 - 99 new samples each
    if name == "classes_9x9":
        assert np.all(k.apod[:, k.cls == 2] == 0) and len(k.pos_m) > 64


# ---- invariants ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_unit_tap_is_the_plain_plan_bit_for_bit(ctx):
    vox = pc.case("unit_tap").trace_voxels()
    plain, ptr = pc.run_device(ctx, "unit_tap", response=False, trace=vox)
    unit, utr = pc.run_device(ctx, "unit_tap", trace=vox)
    assert "response: 1 classes, 1 taps" in unit["variant"] and "response" not in plain["variant"]
    for key in ("pmax", "pmag", "intensity", "pii"):
        assert np.array_equal(plain[key], unit[key]), key
    assert np.array_equal(ptr, utr) and np.abs(ptr).max() > 0


@pytest.mark.gpu
def test_delayed_unit_tap_is_the_plain_plan_three_steps_later(ctx):
    k = pc.case("delayed_unit_tap")
    vox = k.trace_voxels()
    resp, rtr = pc.run_device(ctx, "delayed_unit_tap", trace=vox)
    later = (np.floor(k.delays / k.dt) + 3.5) * k.dt
    plain, ptr = pc.run_device(ctx, "delayed_unit_tap", response=False, delays=later, trace=vox)
    for key, tol in (("pmax", P_TOL), ("pmag", P_TOL), ("pii", PII_TOL)):
        assert np.abs(resp[key].astype(np.float64) - plain[key]).max() <= tol * plain[key].max(), key
    assert np.abs(rtr.astype(np.float64) - ptr).max() <= TRACE_TOL * np.abs(ptr).max()


@pytest.mark.gpu
def test_repeated_launch_and_cleared_response(ctx):
    vox = pc.case("ring30").trace_voxels()
    once, tr1 = pc.run_device(ctx, "ring30", trace=vox)
    twice, tr2 = pc.run_device(ctx, "ring30", trace=vox, launches=2)
    for key in ("pmax", "pmag", "intensity", "pii"):
        assert np.array_equal(once[key], twice[key]), key
    assert np.array_equal(tr1, tr2)
    # run_device has cleared the response (n_classes = 0): the next plan is a fresh context's plain plan
    after, atr = pc.run_device(ctx, "ring30", response=False, trace=vox)
    with nat.Context(0) as fresh:
        ref, ftr = pc.run_device(fresh, "ring30", response=False, trace=vox)
    assert after["variant"] == ref["variant"] and "response" not in ref["variant"]
    for key in ("pmax", "pmag", "intensity", "pii"):
        assert np.array_equal(after[key], ref[key]), key
        assert not np.array_equal(after[key], once[key]), key
    assert np.array_equal(atr, ftr)


def _plain(a):
    return repr(a.to_dict() if hasattr(a, "to_dict") else vars(a))


@pytest.mark.gpu
def test_response_setting_leaves_cw_and_thermal_objects_untouched():
    arr = ol.Transducer.gen_matrix_array(nx=4, ny=4, pitch=2.1, kerf=0.2, units="mm", sensitivity=1e5)
    setup = ol.SimSetup(spacing=1.0, x_extent=(-8, 8), y_extent=(-8, 8), z_extent=(4, 20))
    proto = ol.Protocol(pulse=ol.Pulse(frequency=F0, duration=2e-5), sequence=ol.Sequence(pulse_interval=0.1, pulse_count=2, pulse_train_interval=1.0, pulse_train_count=1),
                        focal_pattern=ol.focal_patterns.Wheel(center=False, num_spokes=2, spoke_radius=1.5, target_pressure=1e6), sim_setup=setup)
    sol, _, _ = proto.calc_solution(ol.Point(position=(0, 0, 12), units="mm"), arr, simulate=True, scale=True)
    run_thermal_simulation(setup.setup_sim_scene(proto.seg_method), sol)
    eng = ol.get_engine()
    variant = eng.ctx.field_variant()
    before = (eng.ctx.field_fetch_all(), eng.ctx.thermal_fetch(), _plain(sol.analyze()))
    eng.ctx.field_pulse_response(np.zeros(16, dtype=np.int32), [pc.damped_sine(30, pc.DT0)])      # continuous-wave plans ignore it
    try:
        assert sol._device_is_current() and eng.ctx.field_variant() == variant
        after = (eng.ctx.field_fetch_all(), eng.ctx.thermal_fetch(), _plain(sol.analyze()))
        eng.ctx.field_launch()
        again = eng.ctx.field_fetch_all()
    finally:
        eng.ctx.field_pulse_response()
    eng.ctx.field_launch()
    assert np.array_equal(again["pmag"], eng.ctx.field_fetch_all()["pmag"])
    for key in ("pmag", "intensity"):
        assert np.array_equal(before[0][key], after[0][key]), key
    for a, b in zip(before[1], after[1]):
        assert np.array_equal(a, b)
    assert before[2] == after[2]


# ---- refusals on the device side -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_response_refusals(ctx):
    k = pc.case("ring30")
    g = k.taps[0]
    with nat.Context(0) as fresh:
        with pytest.raises(nat.NativeError, match="olx_set_elements"):
            fresh.n_el = 16
            fresh.field_pulse_response(k.cls, [g])
    ctx.set_elements(k.pos_m, np.tile([0.0, 0.0, 1.0], (16, 1)), k.area)
    bad = k.cls.copy(); bad[5] = 1
    with pytest.raises(ValueError, match="class"):
        ctx.field_pulse_response(bad, [g])
    bad[5] = -1
    with pytest.raises(ValueError, match="class"):
        ctx.field_pulse_response(bad, [g])
    with pytest.raises(ValueError, match="strictly increasing"):
        ctx.field_pulse_response(k.cls, [g, np.zeros(0)])
    with pytest.raises(ValueError, match="256"):
        ctx.field_pulse_response(k.cls, [np.ones(257)])
    with pytest.raises(ValueError, match="at most"):
        ctx.field_pulse_response(k.cls, [g] * 5)
    for value in (np.nan, np.inf):
        with pytest.raises(ValueError, match="finite"):
            ctx.field_pulse_response(k.cls, [np.array([1.0, value])])
    row = np.array([1, 3], dtype=np.int32)          # (the binding always starts its row table at 0)
    ip = nat.POINTER(nat.c_int32)
    assert ctx._lib.olx_field_pulse_response(ctx._h, 1, k.cls.ctypes.data_as(ip), row.ctypes.data_as(ip), nat._dptr(np.ones(3))) == nat.OLX_EINVAL
    # a refused call keeps nothing: the next pulsed plan is plain
    ctx.set_steering(k.delays, k.apod)
    ctx.field_pulse(k.cycles, k.dt, k.n_t)
    try:
        ctx.field_plan((k.xs[0], k.ys[0], k.zs[0]), k.sp, k.n, F0, C, RHO, P0, flags=nat.OUT_PMAG | nat.OUT_PMAX)
        assert "response" not in ctx.field_variant()
        # a plan that carries a response refuses a medium (kernel 2ph is out of scope)
        ctx.field_pulse_response(k.cls, [g])
        ctx.field_plan((k.xs[0], k.ys[0], k.zs[0]), k.sp, k.n, F0, C, RHO, P0, flags=nat.OUT_PMAG | nat.OUT_PMAX)
        assert ctx.field_variant().endswith("; response: 1 classes, 30 taps")
        with pytest.raises(ValueError, match="impulse response"):
            ctx.field_pulse_medium(np.full(k.n, 1600.0, dtype=np.float32))
        # olx_set_elements clears it, as it clears the apertures
        ctx.set_elements(k.pos_m, np.tile([0.0, 0.0, 1.0], (16, 1)), k.area)
        ctx.set_steering(k.delays, k.apod)
        ctx.field_plan((k.xs[0], k.ys[0], k.zs[0]), k.sp, k.n, F0, C, RHO, P0, flags=nat.OUT_PMAG | nat.OUT_PMAX)
        assert "response" not in ctx.field_variant()
        # continuous-wave plans ignore it
        ctx.field_pulse_response(k.cls, [g])
        ctx.field_pulse(0.0, 0.0, 0)
        ctx.field_plan((k.xs[0], k.ys[0], k.zs[0]), k.sp, k.n, F0, C, RHO, P0, flags=nat.OUT_PMAG)
        assert "response" not in ctx.field_variant()
    finally:
        ctx.field_pulse_response()
        ctx.field_pulse(0.0, 0.0, 0)


# ---- run_simulation and Protocol.calc_solution -----------------------------------------------------------------------------------------
def _array(response=True):
    arr = ol.Transducer.gen_matrix_array(nx=4, ny=4, pitch=3, kerf=0.3, units="mm", sensitivity=1e5)
    if response:
        arr.impulse_response, arr.impulse_dt = pc.damped_sine(12, 2.5e-7), 2.5e-7
        for e in (2, 7):
            arr.elements[e].impulse_response = np.array([0.5])
    return arr


@pytest.mark.gpu
def test_run_simulation_with_the_drive_model():
    arr = _array()
    # (extents off the lattice of exact arrivals, by test_gpu_pulsed.py's SHIFT)
    setup = ol.SimSetup(spacing=0.5, x_extent=(-2.9269, 3.0731), y_extent=(-2.5419, 2.4581), z_extent=(4.0263, 11.0263), t_end=2e-5)
    params = setup.setup_sim_scene(ol.seg.seg_methods.UniformWater())
    with pytest.raises(NotImplementedError, match="impulse_response"):
        sf.run_simulation(arr, params, freq=F0, cycles=3, t_end=2e-5, field_model="pulsed")
    pt = np.array([[0.0, 0.0, 8.0]])
    ds_, raw = sf.run_simulation(arr, params, freq=F0, cycles=3, t_end=2e-5, field_model="pulsed", drive_model="impulse_response",
                                 pulse_intensity_integral=True, record_points=pt)
    assert "response: 2 classes" in ol.get_engine().ctx.field_variant()
    xs, ys, zs = (np.asarray(c.data) * 1e-3 for c in params.coords.values())
    pos_m, _, area, _, _ = arr.element_table()
    area = area * np.array([1.0 if el.sensitivity is None else el.sensitivity for el in arr.elements])
    dt, n_t = sf.pulse_time_axis([0.5e-3] * 3, (len(xs), len(ys), len(zs)), 0.0, 2e-5, 0.5)
    cls, taps = sf.drive_taps(arr, dt)
    X, Y, Z = np.meshgrid(xs, ys, zs, indexing="ij")
    pts = np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1)
    ref = pro.response_volumes(pts, pos_m, area, np.zeros(16), np.ones(16), cls, taps, F0, C, RHO, 1e5, 3, dt, n_t, 0.25e-3)
    ok = ref["margin"] >= MARGIN
    assert (~ok).mean() <= 1e-3
    for key, name, tol in (("p_max", "pmax", P_TOL), ("p_min", "pmin", P_TOL), ("pulse_intensity_integral", "pii", PII_TOL)):
        assert np.abs(np.asarray(ds_[key].data).ravel() - ref[name])[ok].max() <= tol * ref[name].max(), key
    v = int(raw["trace_voxels"][0])
    assert raw["p_trace"].shape == (1, n_t) and np.abs(raw["p_trace"][0] - ref["p"][v]).max() <= TRACE_TOL * np.abs(ref["p"]).max() or not ok[v]
    # without any response the opt-in runs the plain kernel
    bare, _ = sf.run_simulation(_array(False), params, freq=F0, cycles=3, t_end=2e-5, field_model="pulsed", drive_model="impulse_response")
    assert "response" not in ol.get_engine().ctx.field_variant()
    plain, _ = sf.run_simulation(_array(False), params, freq=F0, cycles=3, t_end=2e-5, field_model="pulsed")
    assert np.array_equal(np.asarray(bare["p_max"].data), np.asarray(plain["p_max"].data))
    assert not np.array_equal(np.asarray(ds_["p_max"].data), np.asarray(plain["p_max"].data))


@pytest.mark.gpu
def test_calc_solution_with_the_drive_model():
    setup = ol.SimSetup(spacing=1.0, x_extent=(-8, 8), y_extent=(-8, 8), z_extent=(4, 24),
                        options={"field_model": "pulsed", "pulsed_drive_model": "impulse_response", "pulse_intensity_integral": "1"})
    proto = ol.Protocol(pulse=ol.Pulse(frequency=F0, duration=1e-5), sequence=ol.Sequence(pulse_count=2, pulse_train_interval=0),
                        focal_pattern=ol.focal_patterns.Wheel(center=False, num_spokes=2, spoke_radius=2.0, target_pressure=1e6), sim_setup=setup)
    target = ol.Point(position=(0, 0, 14), units="mm")
    sol, agg, analysis = proto.calc_solution(target, _array(), simulate=True, scale=True)
    assert "response: 2 classes" in ol.get_engine().ctx.field_variant()
    assert np.allclose(analysis.mainlobe_pnp_MPa, 1.0, rtol=1e-5)
    res = sol.simulation_result
    assert "pulse_intensity_integral" in res and float(np.asarray(res["pulse_intensity_integral"].data).max()) > 0
    assert not np.array_equal(np.asarray(res["p_max"].data), np.asarray(res["p_min"].data))
    # the same protocol without the opt-in refuses the transducer, in today's words
    setup.options = {"field_model": "pulsed"}
    with pytest.raises(NotImplementedError, match="impulse_response is not implemented"):
        proto.calc_solution(target, _array(), simulate=True, scale=True)
    # ... and a transducer without responses gives a different (bare-burst) field
    bare, _, _ = proto.calc_solution(target, _array(False), simulate=True, scale=False)
    setup.options = {"field_model": "pulsed", "pulsed_drive_model": "impulse_response"}
    rung, _, _ = proto.calc_solution(target, _array(), simulate=True, scale=False)
    assert not np.array_equal(np.asarray(bare.simulation_result["p_min"].data), np.asarray(rung.simulation_result["p_min"].data))


# ---- the debug library -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_response_kernels_stay_inside_their_extents_in_the_debug_library():
    env = dict(os.environ, OLX_LIB_PATH=os.path.join(LIB, "libolx_dbg.so"))
    code = ("import sys; sys.path[:0] = [%r, %r, %r]\n"
            "from openlifu_amd import _native as nat\n"
            "import pulsed_response_cases as pc\n"
            "ctx = nat.Context(0)\n"
            "for name in %r:\n"
            "    out, tr = pc.run_device(ctx, name, trace=pc.case(name).trace_voxels())\n"
            "    assert out['pmax'].max() > 0 and abs(tr).max() > 0, name\n"
            "ctx.sync()\n"
            "print('response debug cases ok')\n") % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "openlifu-python_amd"), GPU_CASES)
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "response debug cases ok" in tail, tail
