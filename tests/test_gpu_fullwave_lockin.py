"""Full-wave lock-in on the MI355X: the lock-in records of kernel 5 (fullwave_pres_k<.., LOCK>, fullwave_receive_k) through the C-ABI
against the fp64 oracle (tests/fullwave_lockin_oracle.py over tests/fullwave_oracle.py) on the case table of tests/fullwave_cases.py, then
run_fullwave_steady_state and delay_methods.TimeReversal end to end on the shrunken wedge scene, the debug library, and the other resident
objects of the context.

Gates (section 5.14's rule: eight times the largest deviation measured on the MI355X, rounded up to one digit, for
fused-multiply-add and ordering differences across compiler versions):
  volume sums C, S as a fraction of the oracle's max hypot(C, S)     measured 5.65e-6 (uniform water, last third of the run)   gate 5e-5
  receiver sums as a fraction of the largest |Z_r|                   measured 4.65e-6 (the same case and window)               gate 4e-5
  TimeReversal delays [cycles] on the shrunken wedge scene           measured 2.54e-8                                          gate 3e-7
The windows late in a run weigh the most: the sums there are 10^-4 of the whole run's, of a field whose rounding noise stems from the burst."""
import os
import subprocess
import sys

import numpy as np
import pytest

import openlifu_amd as ol
from openlifu_amd import _native as nat
from openlifu_amd.seg.material import Material
from openlifu_amd.seg.seg_methods.threshold import SkullThreshold, skull_slab_image
from openlifu_amd.sim import run_fullwave_steady_state, run_thermal_simulation
from openlifu_amd.sim.field import _np_per_m
from openlifu_amd.util import dataset as ds
import fullwave_cases as fc
import fullwave_lockin_cases as lc
import fullwave_lockin_oracle as lo
import fullwave_oracle as fo
import medium_delay_oracle as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "openlifu-python_amd", "lib")
GATE_VOLUME = 5e-5
GATE_RECEIVERS = 4e-5
GATE_DELAYS = 3e-7          # cycles
F0 = lc.F0


@pytest.fixture(scope="module")
def ctx():
    c = nat.Context(0)
    yield c
    c.close()


def windows(steps):
    """the whole run, its last third, a single step, one that starts at step 0"""
    return {"whole": (0, steps), "last_third": (steps - steps // 3, steps // 3), "single": (steps // 2 + 1, 1), "from_zero": (0, steps // 3)}


def check(got, ref, what):
    dev = lc.deviations(got, ref)
    print(what, {k: f"{v:.3e}" for k, v in dev.items()})
    if "volume" in dev:
        assert dev["volume"] <= GATE_VOLUME, (what, dev)
    if "receivers" in dev:
        assert dev["receivers"] <= GATE_RECEIVERS, (what, dev)
    return dev


# ---- parity with the oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", lc.LOCK_CASES)
def test_matches_oracle(ctx, name):
    k = fc.CASES[name]
    assert 200 <= k["steps"] <= 400
    table = lc.receiver_csr(name, lc.receivers(name))
    row = table[0]
    assert len(row) - 1 == 71 and row[3] == row[4] and set(np.diff(row)) >= {0, 1, 8}          # an empty row, on a voxel, off it; two waves
    for label, window in windows(k["steps"]).items():
        ref = lc.lockin_reference(name, window, table)
        _, got = lc.run_device(ctx, name, window, table)
        assert got[0].dtype == np.float32 and got[2].dtype == np.float64 and got[2].shape == (71,)
        check(got, ref, f"{name} / {label} {window}:")
        assert got[2][3] == 0.0 and got[3][3] == 0.0          # the empty row


@pytest.mark.gpu
def test_one_receiver_and_what_is_recorded_is_opt_in(ctx):
    name = "layered"
    k = fc.CASES[name]
    window = windows(k["steps"])["last_third"]
    table = lc.receiver_csr(name, lc.receivers(name))
    base, both = lc.run_device(ctx, name, window, table)
    plain = fc.run_device(ctx, name)
    for a, b in zip(base, plain):          # the lock-in leaves p_max / p_min / sum p^2 / traces as they are
        assert np.array_equal(a, b)
    # volume only, receivers only, and without sum p^2: the same bits
    _, vol_only = lc.run_device(ctx, name, window, None, volume=True)
    assert vol_only[2] is None and vol_only[3] is None and np.array_equal(vol_only[0], both[0]) and np.array_equal(vol_only[1], both[1])
    _, rec_only = lc.run_device(ctx, name, window, table, volume=False)
    assert rec_only[0] is None and np.array_equal(rec_only[2], both[2]) and np.array_equal(rec_only[3], both[3])
    no_sq, got = lc.run_device(ctx, name, window, table, psq=False)
    assert no_sq[2] is None
    for a, b in zip(got, both):
        assert np.array_equal(a, b)
    # R = 1, no empty row
    one = lc.receiver_csr(name, lc.receivers(name)[1:2], empty_row_at=None)
    assert one[0].tolist() == [0, 8]
    _, got1 = lc.run_device(ctx, name, window, one, volume=False)
    check(got1, lc.lockin_reference(name, window, one), "R = 1:")
    assert got1[2][0] == both[2][1] and got1[3][0] == both[3][1]


@pytest.mark.gpu
def test_split_and_repeated_runs_are_bit_identical(ctx):
    name = "layered"
    k = fc.CASES[name]
    window = windows(k["steps"])["last_third"]
    table = lc.receiver_csr(name, lc.receivers(name))
    one = lc.run_device(ctx, name, window, table)
    inside = window[0] + window[1] // 2 + 1
    for split in (inside, window[0], 7):          # inside the window, at its first step, before it
        two = lc.run_device(ctx, name, window, table, split=split)
        for a, b in zip(one[0] + one[1], two[0] + two[1]):
            assert np.array_equal(a, b), split
    again = lc.run_device(ctx, name, window, table)
    for a, b in zip(one[0] + one[1], again[0] + again[1]):
        assert np.array_equal(a, b)


@pytest.mark.gpu
def test_a_run_without_lockin_after_one_with_it_equals_a_fresh_context(ctx):
    name = "uniform_water"
    k = fc.CASES[name]
    lc.run_device(ctx, name, windows(k["steps"])["whole"], lc.receiver_csr(name, lc.receivers(name)))
    after = fc.run_device(ctx, name)
    with pytest.raises(nat.NativeError, match="recorded no lock-in"):          # olx_fullwave_sources cleared it
        ctx._fw_lock_vol = True
        ctx.fullwave_fetch_lockin()
    fresh_ctx = nat.Context(0)
    try:
        fresh = fc.run_device(fresh_ctx, name)
    finally:
        fresh_ctx.close()
    for a, b in zip(after, fresh):
        assert np.array_equal(a, b)


@pytest.mark.gpu
def test_calls_out_of_order_and_bad_arguments():
    c = nat.Context(0)
    try:
        with pytest.raises(nat.NativeError, match="olx_fullwave_sources first"):
            c.fullwave_lockin(F0, 0, 5)
        k = fc.CASES["short_axis"]
        vox = int(np.prod(k["n"]))
        c.fullwave_plan(k["h"], k["n"], k["c"], k["rho"], k["alpha"], k["c_ref"], k["pml"], k["pml_alpha"], k["dt"])
        with pytest.raises(nat.NativeError, match="olx_fullwave_sources first"):
            c.fullwave_lockin(F0, 0, 5)
        c.fullwave_sources([5], [1.0], [0.0], F0, 3, 0, 10)
        for w0, nw in ((-1, 3), (0, 0), (8, 3), (0, 11), (10, 1)):
            with pytest.raises(ValueError, match="outside the run|window"):
                c.fullwave_lockin(F0, w0, nw)
        with pytest.raises(ValueError, match="freq"):
            c.fullwave_lockin(0.0, 0, 5)
        with pytest.raises(ValueError, match="neither"):
            c.fullwave_lockin(F0, 0, 5, volume=False)
        with pytest.raises(ValueError, match="outside the grid"):
            c.fullwave_lockin(F0, 0, 5, row=[0, 1], voxels=[vox], weights=[1.0])
        with pytest.raises(ValueError, match="outside the grid"):
            c.fullwave_lockin(F0, 0, 5, row=[0, 1], voxels=[-1], weights=[1.0])
        with pytest.raises(ValueError, match="not monotone"):
            c.fullwave_lockin(F0, 0, 5, row=[0, 2, 1, 3], voxels=[1, 2, 3], weights=[1.0, 1.0, 1.0])
        with pytest.raises(ValueError, match="last row offset"):
            c.fullwave_lockin(F0, 0, 5, row=[0, 2], voxels=[1, 2, 3], weights=[1.0, 1.0, 1.0])
        with pytest.raises(ValueError, match="finite"):
            c.fullwave_lockin(F0, 0, 5, row=[0, 1], voxels=[1], weights=[np.nan])
        c.fullwave_lockin(F0, 4, 5, volume=True, row=[0, 1], voxels=[5], weights=[1.0])
        with pytest.raises(nat.NativeError, match="nothing run"):
            c.fullwave_fetch_lockin()
        c.fullwave_run(0, 6)
        with pytest.raises(nat.NativeError, match="before the end of the window"):
            c.fullwave_fetch_lockin()
        c.fullwave_run(6, 3)
        vc, vs, rc, rs = c.fullwave_fetch_lockin()
        assert vc.shape == k["n"] and rc.shape == (1,) and abs(rc[0] - float(vc.reshape(-1)[5])) <= 1e-5 * np.abs(vc).max()
        c.fullwave_lockin(F0, 4, 5, volume=False, row=[0, 1], voxels=[5], weights=[1.0])          # a new lock-in: the records belong to the next run
        with pytest.raises(nat.NativeError, match="nothing run"):
            c.fullwave_fetch_lockin()
        with pytest.raises(nat.NativeError, match="does not continue"):
            c.fullwave_run(9, 1)
        c.fullwave_run(0, 10)
        c._fw_lock_vol = True
        with pytest.raises(nat.NativeError, match="did not record the lock-in volume"):
            c.fullwave_fetch_lockin()
        c._fw_lock_vol = False
        c.fullwave_lockin(F0, 4, 5, volume=True)
        c.fullwave_run(0, 10)
        c._fw_lock_nrec = 1
        with pytest.raises(nat.NativeError, match="did not record receivers"):
            c.fullwave_fetch_lockin()
        c.sync()
    finally:
        c.close()


# ---- end to end on the shrunken wedge scene -------------------------------------------------------------------------------------------
RAMP, SETTLE, LOCKIN = 1.0, 1.0, 3.0


def _wedge_product_scene():
    """The shrunken wedge scene as the product sees it: ``params`` on the interior grid (mm, x = y = 0 on the array's axis, z = 0 its first
    plane), a 4 x 4 array at z = 0 moved onto the scene's elements by ``transform``, the target on the scene's focus voxel -> (arr, params,
    transform, target, scene with the elements where the transform puts them)"""
    sc = lc.small_wedge()
    h, q, half = sc["h"], sc["pml"], sc["half"]
    nz = sc["n"][2] - 2 * q
    setup = ol.SimSetup(spacing=h * 1e3, x_extent=(-half * h * 1e3, half * h * 1e3), y_extent=(-half * h * 1e3, half * h * 1e3), z_extent=(0, (nz - 1) * h * 1e3))
    params = setup.setup_sim_scene(ol.seg_methods.UniformWater())
    crop = (slice(q, -q),) * 3
    vols = {"sound_speed": sc["c"][crop], "density": sc["rho"][crop], "attenuation": sc["alpha"][crop] / _np_per_m(1.0, F0)}
    for key, vol in vols.items():
        assert vol.shape == np.asarray(params[key].data).shape
        params[key] = ds.make_dataarray(vol, coords=params.coords, dims=list(params.coords.keys()), name=key, attrs=dict(params[key].attrs))
    assert float(params["sound_speed"].attrs["ref_value"]) == lc.C0
    arr = ol.Transducer.gen_matrix_array(nx=4, ny=4, pitch=1.0, kerf=0.1, units="mm", sensitivity=1e5)
    M = np.eye(4); M[:3, 3] = [0.2 * h, 0.35 * h, 1.5 * h]
    shift = np.array([(q + half) * h, (q + half) * h, q * h])
    sc = dict(sc, pos=arr.element_table()[0] + M[:3, 3] + shift, shift=shift)
    target = ol.Point(position=tuple((sc["focus"] - shift) * 1e3), units="mm")
    return arr, params, M, target, sc


def _product_axis(sc, extra_delay=0.0, ramp=RAMP, settle=SETTLE, lockin=LOCKIN):
    """The time axis run_fullwave_steady_state gives itself: t_end = |n h| / c_min + max tau + (ramp + settle + lockin) / f0 on the interior grid"""
    interior = np.asarray(sc["n"]) - 2 * sc["pml"]
    t_end = np.sqrt(np.sum((interior * sc["h"]) ** 2)) / lc.C0 + extra_delay + (ramp + settle + lockin) / F0
    n_steps = int(np.ceil(t_end / sc["dt"]))
    return (n_steps, lo.drive_cycles(F0, t_end)) + lo.window_of(n_steps, sc["dt"], F0, lockin)


@pytest.mark.gpu
def test_time_reversal_delays_match_the_oracle():
    arr, params, M, target, sc = _wedge_product_scene()
    axis = _product_axis(sc)
    assert 200 <= axis[0] <= 400
    # the oracle, on the scene's whole grid; the anchor on the interior grid, as StraightRay sees it
    Z = lc.listen(sc, axis, ramp=RAMP)
    q = sc["pml"]
    crop = (slice(q, -q),) * 3
    ray = mo.delays(sc["pos"] - sc["shift"], (sc["focus"] - sc["shift"])[None], sc["c"][crop], -np.array([sc["half"], sc["half"], 0]) * sc["h"], (sc["h"],) * 3, lc.C0)[0]
    ref, margin, m, _ = lo.time_reversal(Z, ray, F0)
    assert margin >= 0.25                          # a condition on the input: no element near a wrap
    assert np.abs(ref - lc.direct_delays(sc)).max() * F0 > 0.05          # the slab matters
    method = ol.delay_methods.TimeReversal(frequency=F0, lockin_cycles=LOCKIN, settle_cycles=SETTLE, ramp_cycles=RAMP, pml_size=q)
    delays, amps, info = method.solve(arr, target, params, transform=M)
    raw = info["raw"][0]
    assert raw["n_steps"] == axis[0] and raw["window"] == axis[2:] and raw["dt"] == pytest.approx(sc["dt"], rel=1e-14)
    dev_z = np.abs(raw["receiver_sums"] - Z).max() / np.abs(Z).max()
    dev = np.abs(delays[0] - ref).max() * F0
    print(f"TimeReversal on the shrunken wedge: delays {dev:.3e} cycles, receiver sums {dev_z:.3e} of the largest, tie margin {info['tie_margin'][0]:.3f} (oracle {margin:.3f})")
    assert dev_z <= GATE_RECEIVERS
    assert dev <= GATE_DELAYS
    assert np.array_equal(info["cycles"][0], m) and info["tie_margin"][0] == pytest.approx(margin, abs=1e-4)
    assert np.abs(amps[0] - 2.0 / axis[3] * np.abs(Z)).max() <= GATE_RECEIVERS * (2.0 / axis[3] * np.abs(Z)).max()
    assert np.array_equal(method.calc_delays(arr, target, params, transform=M), delays[0])          # the public method; and a repeated run is the same run
    by_direct = ol.delay_methods.TimeReversal(frequency=F0, lockin_cycles=LOCKIN, settle_cycles=SETTLE, ramp_cycles=RAMP, pml_size=q, anchor="direct")
    assert np.abs(by_direct.calc_delays(arr, target, params, transform=M) - delays[0]).max() * F0 <= 1e-9          # either anchor: the same whole cycles
    # through the plug-in path of a Protocol, at the pulse's frequency
    proto = ol.Protocol(pulse=ol.Pulse(frequency=F0, duration=2e-5),
                        delay_method=ol.delay_methods.TimeReversal(lockin_cycles=LOCKIN, settle_cycles=SETTLE, ramp_cycles=RAMP, pml_size=q))
    moved = ol.Transducer.gen_matrix_array(nx=4, ny=4, pitch=1.0, kerf=0.1, units="mm", sensitivity=1e5)
    d0, a0 = proto.beamform(moved, target, params)          # (no transform on this path: the array sits on the first plane, on the voxels' rows)
    assert d0.shape == (16,) and a0.shape == (16,) and d0.min() == 0.0 and np.isfinite(d0).all()


@pytest.mark.gpu
def test_steady_state_end_to_end():
    arr, params, M, target, sc = _wedge_product_scene()
    h, q = sc["h"], sc["pml"]
    # elements on the array's own positions (no transform on this seam): off the voxels in x and y, on the first plane
    pos = arr.element_table()[0] + sc["shift"]
    d = np.sqrt(((pos - sc["focus"]) ** 2).sum(axis=1))
    delays = (d.max() - d) / lc.C0 + 0.37e-7
    apod = np.ones(16); apod[5] = 0.0; apod[9] = 0.5
    rec = np.array([[0.0, 0.0, 1.5], [0.3, -0.7, 2.1]])
    out, raw = run_fullwave_steady_state(arr, params, delays, apod, freq=F0, amplitude=2.0, lockin_cycles=LOCKIN, settle_cycles=SETTLE, ramp_cycles=RAMP,
                                         pml_size=q, receivers=rec)
    axis = _product_axis(sc, extra_delay=delays.max())
    assert raw["n_steps"] == axis[0] and raw["window"] == axis[2:] and raw["cycles"] == axis[1] and 200 <= axis[0] <= 400
    assert raw["backend"] == "openlifu_amd/hip-gfx950" and raw["points_per_wavelength"] == pytest.approx(1500.0 / (F0 * h))
    area = arr.element_table()[2]
    A0 = apod * area * 2.0 * 1e5 * F0 / lc.C0
    src = fo.monopole_entries(pos, (0, 0, 0), h, A0, delays, sc["c"], F0, sc["dt"], sc["n"])
    assert fo.activity_margin(src[2], axis[1] / F0, sc["dt"]) >= 1e-6
    every = np.stack(np.meshgrid(*[np.arange(v) for v in sc["n"]], indexing="ij"), axis=-1).reshape(-1, 3)
    Zr, tr = lo.steady_receivers(sc["n"], h, sc["c"], sc["rho"], sc["alpha"], lc.C0, q, 2.0, sc["dt"], axis[0], src, rec * 1e-3 + sc["shift"], F0, axis[1], RAMP,
                                 axis[2], axis[3], trace_extra=every)
    C, S = lo.volume_sums(tr, F0, sc["dt"], axis[2], axis[3])
    crop = (slice(q, -q),) * 3
    A, psi = lo.amplitude_phase(C.reshape(sc["n"])[crop], S.reshape(sc["n"])[crop], axis[3])
    got_A, got_psi = np.asarray(out["p_max"].data), np.asarray(out["phase"].data)
    assert got_A.dtype == np.float32 and got_A.shape == A.shape and out["phase"].attrs["units"] == "cycles" and out["p_min"].attrs["units"] == "Pa"
    assert np.array_equal(got_A, np.asarray(out["p_min"].data))
    dev_a = np.abs(got_A - A).max() / A.max()
    dev_p = np.abs(got_A * np.exp(2j * np.pi * got_psi) - A * np.exp(2j * np.pi * psi)).max() / A.max()
    dev_r = np.abs(raw["receiver_sums"] - Zr).max() / np.abs(Zr).max()
    print(f"steady state end to end: amplitude {dev_a:.3e}, amplitude x phase {dev_p:.3e} of the largest amplitude; receiver sums {dev_r:.3e}")
    # float32 outputs: half an ulp of the amplitude, and of the phase (at most 1/2 cycle) times 2 pi, on top of the sums' gate
    assert dev_a <= GATE_VOLUME + 2.0 ** -24
    assert dev_p <= GATE_VOLUME + (1 + np.pi) * 2.0 ** -24
    assert dev_r <= GATE_RECEIVERS
    assert np.all((got_psi > -0.5) & (got_psi <= 0.5))
    ra, rp = lo.amplitude_phase(Zr.real, Zr.imag, axis[3])
    assert np.allclose(raw["receiver_amplitude"], ra, rtol=0, atol=GATE_RECEIVERS * ra.max())
    inten = 1e-4 * A ** 2 / (2 * sc["rho"][crop] * sc["c"][crop])
    assert out["intensity"].attrs["units"] == "W/cm^2"
    assert np.abs(np.asarray(out["intensity"].data) - inten).max() <= 4 * GATE_VOLUME * inten.max()
    fi = tuple(sc["focus_ijk"] - q)
    assert got_A[fi] > 0          # the wave reached the focus


# ---- a steady-state run changes nothing else ------------------------------------------------------------------------------------------
def _assert_same_analysis(a, b):
    """Equal field by field; the focal centroids to rounding only -- their fp64 block sums are added with atomicAdd in the order the blocks
    arrive (field_masked_moments_k), so two analyses of the same bits may differ in the last digit."""
    da, db = (x.to_dict() if hasattr(x, "to_dict") else dict(vars(x)) for x in (a, b))
    assert list(da) == list(db)
    for key in da:
        if key.startswith("focal_centroid"):
            assert np.allclose(np.asarray(da[key], dtype=np.float64), np.asarray(db[key], dtype=np.float64), rtol=1e-12, atol=1e-12), key
        else:
            assert repr(da[key]) == repr(db[key]), key


@pytest.mark.gpu
def test_steady_state_run_leaves_the_other_resident_objects_untouched():
    arr = ol.Transducer.gen_matrix_array(nx=4, ny=4, pitch=2.1, kerf=0.2, units="mm", sensitivity=1e5)
    setup = ol.SimSetup(spacing=0.5, x_extent=(-6, 6), y_extent=(-6, 6), z_extent=(0, 16))
    mats = {"water": Material("water", 1500.0, 1000.0, 0.0022, 4182.0, 0.598), "skull": Material("skull", 2800.0, 1900.0, 6.0, 1300.0, 0.4)}
    proto = ol.Protocol(pulse=ol.Pulse(frequency=F0, duration=2e-5), sequence=ol.Sequence(pulse_interval=0.1, pulse_count=2, pulse_train_interval=1.0, pulse_train_count=1),
                        focal_pattern=ol.focal_patterns.Wheel(center=False, num_spokes=2, spoke_radius=1.5, target_pressure=1e6),
                        sim_setup=setup, seg_method=SkullThreshold(materials=mats), apod_method=ol.apod_methods.Uniform())
    coords = setup.get_coords()
    xs, ys, zs = (np.asarray(c.data) * 1e-3 for c in coords.values())
    dims = list(coords.keys() if not hasattr(coords, "dims") else coords.dims)
    vol = ds.make_dataarray(skull_slab_image(xs, ys, zs), coords=coords, dims=dims, name="ct")
    sol, _, _ = proto.calc_solution(ol.Point(position=(0, 0, 12), units="mm"), arr, volume=vol, simulate=True, scale=True)
    params = setup.setup_sim_scene(proto.seg_method, volume=vol)
    run_thermal_simulation(params, sol)
    eng = ol.get_engine()
    assert sol._device_is_current()
    variant = eng.ctx.field_variant()
    before = (eng.ctx.field_fetch_all(), eng.ctx.thermal_fetch(), sol.analyze())
    run_fullwave_steady_state(arr, params, sol.delays[0], sol.apodizations[0], freq=F0, lockin_cycles=2, settle_cycles=0.5, ramp_cycles=1.0, t_end=1.4e-5, pml_size=6,
                              receivers=[[0.0, 0.0, 12.0]])
    assert sol._device_is_current() and eng.ctx.field_variant() == variant
    after = (eng.ctx.field_fetch_all(), eng.ctx.thermal_fetch(), sol.analyze())
    for key in ("pmag", "intensity"):
        assert np.array_equal(before[0][key], after[0][key]), key
    for a, b in zip(before[1], after[1]):
        assert np.array_equal(a, b)
    _assert_same_analysis(before[2], after[2])
    eng.ctx.field_launch()
    again = eng.ctx.field_fetch_all()
    eng.ctx.field_launch()
    assert np.array_equal(again["pmag"], eng.ctx.field_fetch_all()["pmag"])


# ---- the debug library --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_lockin_kernels_stay_inside_their_extents_in_the_debug_library():
    env = dict(os.environ, OLX_LIB_PATH=os.path.join(LIB, "libolx_dbg.so"))
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "from openlifu_amd import _native as nat\n"
            "import fullwave_cases as fc, fullwave_lockin_cases as lc\n"
            "ctx = nat.Context(0)\n"
            "for name in lc.LOCK_CASES:\n"
            "    steps = fc.CASES[name]['steps']\n"
            "    table = lc.receiver_csr(name, lc.receivers(name))\n"
            "    for window in ((0, steps), (steps - steps // 3, steps // 3), (steps // 2 + 1, 1)):\n"
            "        dev = lc.deviations(lc.run_device(ctx, name, window, table)[1], lc.lockin_reference(name, window, table))\n"
            "        assert dev['volume'] <= %r and dev['receivers'] <= %r, (name, window, dev)\n"
            "lc.run_device(ctx, 'layered', (300, 100), lc.receiver_csr('layered', lc.receivers('layered')), split=337)\n"
            "ctx.sync()\n"
            "print('fullwave lock-in debug cases ok')\n") % (os.path.join(ROOT, "tests"), os.path.join(ROOT, "openlifu-python_amd"), GATE_VOLUME, GATE_RECEIVERS)
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "fullwave lock-in debug cases ok" in tail, tail
