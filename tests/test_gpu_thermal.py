"""Thermal model on the MI355X: kernel 3 (thermal_pack_k / thermal_step_k) through the C-ABI against the fp64 oracle of the same
discrete scheme (tests/thermal_oracle.py), known answers on the device result, the resident intensity read in place, and
run_thermal_simulation after Protocol.calc_solution end to end.
Gate (DESIGN.md section 2 "thermal model"): temperature_rise_max and traces <= 1e-4 of the volume maximum; CEM43 <= 1e-3 relative
wherever it exceeds 1e-3 of its maximum."""
import os
import subprocess
import sys

import numpy as np
import pytest

import openlifu_amd as ol
from openlifu_amd import _native as nat
from openlifu_amd.sim import run_thermal_simulation
from openlifu_amd.sim import thermal as th
from openlifu_amd.seg.seg_methods.threshold import SkullThreshold, skull_slab_image
from openlifu_amd.seg.material import Material
from openlifu_amd.util import dataset as ds
import thermal_oracle as to

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "openlifu-python_amd", "lib")
# the example protocol's materials (tests/golden/example_db/example_protocol.json)
WATER = (1000.0, 4182.0, 0.598, 0.0022)
SKULL = (1900.0, 1300.0, 0.4, 6.0)
TISSUE = (1050.0, 3600.0, 0.528, 0.3)
FREQ = 500e3


@pytest.fixture(scope="module")
def ctx():
    c = nat.Context(0)
    yield c
    c.close()


def _np_m(db):
    return np.asarray(db, dtype=np.float64) * th._np_per_m(1.0, FREQ)


def layered(shape, axis_z=2):
    """water / skull / tissue along z, as float volumes (rho, cp, kappa, attenuation [dB/cm/MHz])."""
    nz = shape[axis_z]
    lab = np.zeros(shape, dtype=int)
    lab[..., nz // 3: nz // 2] = 1
    lab[..., nz // 2:] = 2
    mats = np.array([WATER, SKULL, TISSUE])
    return tuple(mats[lab, q] for q in range(4))


def gaussian_sources(shape, centres, sigma_vox, peak=50.0):
    idx = np.indices(shape).astype(np.float64)
    out = np.empty((len(centres),) + shape, dtype=np.float32)
    for f, c in enumerate(centres):
        r2 = sum((idx[a] - c[a]) ** 2 for a in range(3))
        out[f] = peak * np.exp(-r2 / (2 * sigma_vox ** 2))
    return out


def check_gate(got, ref):
    rise, cem, tr = got
    rr, rc, rt = ref[:3]
    scale = np.abs(rr).max()
    assert scale > 0
    assert np.abs(rise - rr).max() <= 1e-4 * scale, np.abs(rise - rr).max() / scale
    if rt.size:
        assert np.abs(tr - rt).max() <= 1e-4 * scale, np.abs(tr - rt).max() / scale
    m = rc > 1e-3 * rc.max()
    rel = np.abs(cem[m] - rc[m]) / rc[m]
    assert rel.max() <= 1e-3, rel.max()


def run_case(ctx, shape, h, medium, inten, sched, dt, n_steps, baseline=37.0, perfusion=0.0, points=None):
    rho, cp, kap, att = medium
    alpha = _np_m(att)
    ctx.thermal_plan((0.0, 0.0, 0.0), h, shape, rho, cp, kap, alpha if np.ndim(alpha) else float(alpha), perfusion=perfusion)
    ctx.thermal_schedule(*sched, points=points)
    ctx.thermal_source(inten.shape[0], inten)
    ctx.thermal_run(dt, baseline)
    got = ctx.thermal_fetch()
    ref = to.run(rho, cp, kap, alpha, inten, h, *sched, dt, n_steps, baseline=baseline, perfusion=perfusion, points=points)
    return got, ref


def pulsed_sched(F, dt, n_steps, duration, interval, count, train=0.0, trains=1):
    pulse = ol.Pulse(frequency=FREQ, duration=duration)
    seq = ol.Sequence(pulse_interval=interval, pulse_count=count, pulse_train_interval=train, pulse_train_count=trains)
    return th.thermal_schedule(pulse, seq, F, dt, n_steps)


CASES = {
    "water_uniform_1focus": dict(shape=(32, 32, 32), h=(0.5e-3,) * 3, layered=False, foci=1, perfusion=0.0, steps=60, points=False),
    "skull_layers_odd_aniso_3foci": dict(shape=(41, 37, 53), h=(0.4e-3, 0.5e-3, 0.3e-3), layered=True, foci=3, perfusion=0.0, steps=80, points=True),
    "skull_layers_perfusion": dict(shape=(24, 20, 30), h=(0.5e-3,) * 3, layered=True, foci=1, perfusion=2e4, steps=70, points=True),
    "water_to_the_boundary": dict(shape=(16, 12, 14), h=(0.25e-3,) * 3, layered=False, foci=3, perfusion=0.0, steps=400, points=True),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_thermal_kernel_matches_oracle(ctx, name):
    cs = CASES[name]
    shape, h = cs["shape"], cs["h"]
    medium = layered(shape) if cs["layered"] else WATER
    F = cs["foci"]
    centres = [tuple(s // 2 + d for s in shape) for d in (0, 2, -3)][:F]
    inten = gaussian_sources(shape, centres, 2.0, peak=200.0 if cs["layered"] else 2000.0)
    rho, cp, kap, _ = (np.broadcast_to(np.asarray(v, dtype=np.float64), shape) for v in medium)
    dt = 0.5 * to.ftcs_bound(rho, cp, kap, h, shape, cs["perfusion"])
    n_steps = cs["steps"]
    # pulses of 0.3 dt every 0.7 dt (they straddle step boundaries), foci in get_ita's order
    sched = pulsed_sched(F, dt, n_steps, 0.3 * dt, 0.7 * dt, count=6 * F + 1, train=0.0, trains=n_steps // (6 * F + 1) + 1)
    pts = None
    if cs["points"]:
        pts = np.array([np.ravel_multi_index(c, shape) for c in centres] + [0, int(np.prod(shape)) - 1])
    got, ref = run_case(ctx, shape, h, medium, inten, sched, dt, n_steps, perfusion=cs["perfusion"], points=pts)
    check_gate(got, ref)
    if name == "water_to_the_boundary":          # long enough that heat reaches the boundary
        assert np.abs(ref[3][0]).max() > 1e-3 * ref[3].max()


@pytest.mark.gpu
def test_thermal_cem43_above_43(ctx):
    shape, h = (20, 20, 20), (0.5e-3,) * 3
    inten = gaussian_sources(shape, [(10, 10, 10)], 2.5, peak=30.0)
    dt = 0.5 * to.ftcs_bound(1000.0, 4182.0, 0.598, h, shape)
    n_steps = 120
    sched = (np.arange(n_steps + 1, dtype=np.int32), np.zeros(n_steps, dtype=np.int32), np.full(n_steps, dt))
    got, ref = run_case(ctx, shape, h, (1000.0, 4182.0, 0.598, 1.0), inten, sched, dt, n_steps, baseline=41.0)
    assert 3.0 < ref[0].max() < 10.0            # crosses 43 degC: both branches of R
    check_gate(got, ref)


@pytest.mark.gpu
def test_thermal_gaussian_and_energy_on_device(ctx):
    sigma, h, n = 1e-3, 0.25e-3, 41
    x = (np.arange(n) - n // 2) * h
    r2 = x[:, None, None] ** 2 + x[None, :, None] ** 2 + x[None, None, :] ** 2
    q0, alpha = 2e6, 10.0
    inten = (q0 * np.exp(-r2 / (2 * sigma ** 2)) / (2 * alpha * 1e4))[None].astype(np.float32)
    dt_max = to.ftcs_bound(1000.0, 4182.0, 0.598, (h,) * 3, r2.shape)
    n_steps = int(np.ceil(1.0 / (dt_max / 2)))
    dt = 1.0 / n_steps
    sched = (np.arange(n_steps + 1, dtype=np.int32), np.zeros(n_steps, dtype=np.int32), np.full(n_steps, dt))
    ctx.thermal_plan((0.0,) * 3, (h,) * 3, r2.shape, 1000.0, 4182.0, 0.598, alpha)
    ctx.thermal_schedule(*sched, points=[np.ravel_multi_index((n // 2,) * 3, r2.shape)])
    ctx.thermal_source(1, inten)
    ctx.thermal_run(dt, 37.0)
    rise, _, tr = ctx.thermal_fetch()
    D = 0.598 / (1000.0 * 4182.0)
    tau = np.linspace(0, 1.0, 20001)
    exact = q0 / (1000.0 * 4182.0) * np.trapezoid((sigma ** 2 / (sigma ** 2 + 2 * D * tau)) ** 1.5, tau)
    assert tr[-1, 0] == pytest.approx(exact, rel=1e-2)
    # energy: a few steps from a point source, every voxel traced (the last row is the final state), the boundary still at exactly 0
    m, hm = 21, 0.5e-3
    src = np.zeros((1, m, m, m), dtype=np.float32); src[0, 10, 10, 10] = 100.0
    ctx.thermal_plan((0.0,) * 3, (hm,) * 3, (m, m, m), 1000.0, 4182.0, 0.598, 20.0)
    dt = 0.4 * to.ftcs_bound(1000.0, 4182.0, 0.598, (hm,) * 3, (m, m, m))
    ctx.thermal_schedule(np.arange(9, dtype=np.int32), np.zeros(8, dtype=np.int32), np.full(8, dt), points=np.arange(m ** 3))
    ctx.thermal_source(1, src)
    ctx.thermal_run(dt, 37.0)
    _, _, tr = ctx.thermal_fetch()
    t = tr[-1].astype(np.float64).reshape(m, m, m)
    assert t[0].max() == 0 and t[-1].max() == 0 and t[:, 0].max() == 0 and t[:, :, -1].max() == 0
    deposited = 8 * dt * 2 * 20.0 * 1e4 * float(src.max()) / (1000.0 * 4182.0)
    assert t.sum() == pytest.approx(deposited, rel=1e-5)         # (fp32 state: the sum of 9261 floats)


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def _skull_protocol(seconds=2.0):
    mats = {"water": Material("water", 1500.0, 1000.0, 0.0022, 4182.0, 0.598), "skull": Material("skull", 2800.0, 1900.0, 6.0, 1300.0, 0.4),
            "tissue": Material("tissue", 1540.0, 1050.0, 0.3, 3600.0, 0.528)}
    setup = ol.SimSetup(spacing=0.5, x_extent=(-8, 8), y_extent=(-8, 8), z_extent=(4, 28))
    return ol.Protocol(pulse=ol.Pulse(frequency=FREQ, duration=2e-5),
                       sequence=ol.Sequence(pulse_interval=0.1, pulse_count=10, pulse_train_interval=1.0, pulse_train_count=int(seconds)),
                       focal_pattern=ol.focal_patterns.SinglePoint(target_pressure=1e6), sim_setup=setup,
                       seg_method=SkullThreshold(materials=mats), apod_method=ol.apod_methods.Uniform()), setup


def _volume(setup):
    coords = setup.get_coords()
    xs, ys, zs = (np.asarray(c.data) * 1e-3 for c in coords.values())
    img = skull_slab_image(xs, ys, zs)
    dims = list(coords.keys() if not hasattr(coords, "dims") else coords.dims)
    return ds.make_dataarray(img, coords=coords, dims=dims, name="ct")


def _array():
    return ol.Transducer.gen_matrix_array(nx=8, ny=8, pitch=2, kerf=0.2, units="mm", sensitivity=1e5)


@pytest.mark.gpu
def test_resident_intensity_matches_uploaded_and_stays_unchanged():
    proto, setup = _skull_protocol()
    vol = _volume(setup)
    target = ol.Point(position=(0, 0, 20), units="mm")
    sol, _, _ = proto.calc_solution(target, _array(), volume=vol, simulate=True, scale=True)
    params = setup.setup_sim_scene(proto.seg_method, volume=vol)
    assert sol._device_is_current()
    a_ds, a_raw = run_thermal_simulation(params, sol, record_points=[[0, 0, 20.0]])
    assert a_raw["source"] == "resident"
    pmin, inten = np.array(sol.simulation_result["p_min"].data), np.array(sol.simulation_result["intensity"].data)
    b_ds, b_raw = run_thermal_simulation(params, sol, record_points=[[0, 0, 20.0]])
    assert b_raw["source"] == "uploaded"
    for k in ("temperature_rise_max", "CEM43", "temperature_max"):
        assert np.array_equal(np.asarray(a_ds[k].data), np.asarray(b_ds[k].data)), k
    assert np.array_equal(a_raw["traces"], b_raw["traces"])
    # the same solution computed again, never touched by a thermal run: identical volumes
    sol2, _, _ = proto.calc_solution(target, _array(), volume=vol, simulate=True, scale=True)
    assert np.array_equal(np.array(sol2.simulation_result["p_min"].data), pmin)
    assert np.array_equal(np.array(sol2.simulation_result["intensity"].data), inten)


@pytest.mark.gpu
def test_end_to_end_skull_heats_most():
    proto, setup = _skull_protocol(seconds=2.0)
    vol = _volume(setup)
    target = ol.Point(position=(0, 0, 20), units="mm")
    sol, _, _ = proto.calc_solution(target, _array(), volume=vol, simulate=True, scale=True)
    params = setup.setup_sim_scene(proto.seg_method, volume=vol)
    out, raw = run_thermal_simulation(params, sol)
    tmax = np.asarray(out["temperature_max"].data)
    assert tmax.min() >= 37.0 and out["temperature_max"].attrs["units"] == "degC"
    hot = np.unravel_index(np.argmax(np.asarray(out["temperature_rise_max"].data)), tmax.shape)
    assert np.asarray(vol.data)[hot] >= 300.0, hot          # the hottest voxel is bone
    assert raw["n_steps"] * raw["dt"] == pytest.approx(sol.sequence.get_sequence_duration(), rel=1e-12)
    cems = [np.asarray(out["CEM43"].data)]
    for seconds in (4.0, 6.0):
        p2, _ = _skull_protocol(seconds)
        s2, _, _ = p2.calc_solution(target, _array(), volume=vol, simulate=True, scale=True)
        cems.append(np.asarray(run_thermal_simulation(params, s2)[0]["CEM43"].data))
    assert np.all(cems[1] >= cems[0]) and np.all(cems[2] >= cems[1]) and cems[2].max() > cems[0].max()


# ---- the debug library -----------------------------------------------------------------------------------------------------------
def test_thermal_bounds_tag_only_in_the_debug_library():
    prod = open(os.path.join(LIB, "libolx.so"), "rb").read()
    dbg = open(os.path.join(LIB, "libolx_dbg.so"), "rb").read()
    assert b"olx_dbg_bounds_thermal" in dbg and b"olx_dbg_bounds_thermal" not in prod


@pytest.mark.gpu
def test_thermal_kernels_stay_inside_their_extents_in_the_debug_library():
    env = dict(os.environ, OLX_LIB_PATH=os.path.join(LIB, "libolx_dbg.so"))
    sel = "matches_oracle or cem43_above or gaussian_and_energy"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", sel, "-p", "no:cacheprovider"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=1200)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in tail and "failed" not in tail, tail
