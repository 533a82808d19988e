"""Eikonal travel times on the MI355X: kernel 6 (eikonal_*_k) through the C-ABI against the fp64 oracle of the same discrete scheme
(tests/eikonal_oracle.py) over the case table of tests/eikonal_cases.py -- the full volume, no voxel left out, and 71 sample points --
then the ``Eikonal`` delay method end to end, through ``Protocol.beamform`` and with a transform, in the debug library, and next to the other
resident objects of the context.

Gate: the largest deviation measured over the case table, as a fraction of the oracle's largest T, was 2.53e-7
(the volume of the clipped_low case; samples <= 1.41e-7); the gate is eight times that, rounded up to one digit: 3e-6.  The margin covers
fused-multiply-add and compiler differences.  End to end on scene A at 0.5 mm the largest deviation from the oracle was 9.74e-7 cycles at
500 kHz (extra path and travel time; the delays 7.9e-7, with a transform too); the gate there, by the same rule, is 8e-6 cycles."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import openlifu_amd as ol
from openlifu_amd import _native as nat
from openlifu_amd.bf.delay_methods import Eikonal
from openlifu_amd.seg.material import Material
from openlifu_amd.seg.seg_methods.threshold import SkullThreshold, skull_slab_image
from openlifu_amd.sim import run_thermal_simulation
from openlifu_amd.util import dataset as ds
import eikonal_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "openlifu-python_amd", "lib")
GATE = 3e-6
GATE_CYCLES = 8e-6
FREQ = 500e3


@pytest.fixture(scope="module")
def ctx():
    c = nat.Context(0)
    yield c
    c.close()


def check_gate(got, name):
    dev = ec.deviations(got, name)
    print(name, {k: f"{v:.3e}" for k, v in dev.items()}, "sweeps", got[1])
    for key, v in dev.items():
        assert v <= GATE, (name, key, v)


# ---- parity with the oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ec.CASES))
def test_matches_oracle(ctx, name):
    k = ec.CASES[name]
    got = ec.run_device(ctx, name)
    assert got[0].shape == k["n"] and got[0].dtype == np.float32 and got[2].shape == (71,) and got[2].dtype == np.float64
    check_gate(got, name)
    assert 1 <= got[1] < 4 * sum(k["n"])                     # converged below the default cap
    assert got[0].min() >= 0


@pytest.mark.gpu
def test_one_sample_point(ctx):
    k = ec.CASES["layered"]
    ctx.eikonal_solve(k["origin"], k["h"], k["n"], k["c"], k["src"])
    for p in (ec.points("layered")[1:2], ec.points("layered")[0:1]):          # off the voxels (8 entries), on one (1 entry)
        got = ctx.eikonal_sample(*ec.table("layered", p))
        ref = ec.sample_reference("layered", p)
        assert got.shape == (1,) and abs(got[0] - ref[0]) <= GATE * ec.reference("layered")[0].max()


@pytest.mark.gpu
def test_a_volume_filled_with_the_uniform_speed_gives_the_uniform_bits(ctx):
    k = ec.CASES["layered"]
    tab = ec.table("layered")
    ctx.eikonal_solve(k["origin"], k["h"], k["n"], 1500.0, k["src"])
    uni = (ctx.eikonal_fetch(), ctx.eikonal_sample(*tab))
    ctx.eikonal_solve(k["origin"], k["h"], k["n"], np.full(k["n"], 1500.0, dtype=np.float32), k["src"])
    vol = (ctx.eikonal_fetch(), ctx.eikonal_sample(*tab))
    assert np.array_equal(uni[0], vol[0]) and np.array_equal(uni[1], vol[1])          # E = c_ref (T_med - T_ref) == 0 exactly
    assert np.isfinite(uni[0]).all()


@pytest.mark.gpu
def test_a_repeated_solve_is_bit_identical(ctx):
    a = ec.run_device(ctx, "layered")
    ec.run_device(ctx, "uniform_water")              # (a smaller solve in between)
    b = ec.run_device(ctx, "layered")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and a[1] == b[1]


@pytest.mark.gpu
def test_a_cap_too_low_fails_cleanly_and_the_context_stays_usable(ctx):
    ec.run_device(ctx, "uniform_water")
    with pytest.raises(nat.ConvergenceError, match="no convergence within max_sweeps = 3"):
        ec.run_device(ctx, "layered", max_sweeps=3)
    with pytest.raises(nat.NativeError, match="no converged"):          # never a partial field
        ctx.eikonal_fetch()
    with pytest.raises(nat.NativeError, match="no converged"):
        ctx.eikonal_sample(*ec.table("layered"))
    check_gate(ec.run_device(ctx, "layered"), "layered")
    sweeps = ec.run_device(ctx, "layered")[1]
    assert ec.run_device(ctx, "layered", max_sweeps=sweeps)[1] == sweeps      # the cap counts the last sweep too
    with pytest.raises(nat.ConvergenceError):
        ec.run_device(ctx, "layered", max_sweeps=sweeps - 1)
    ctx.sync()


@pytest.mark.gpu
def test_calls_out_of_order_and_bad_arguments():
    c = nat.Context(0)
    try:
        k = ec.CASES["uniform_water"]
        with pytest.raises(nat.NativeError, match="no converged"):
            c.eikonal_sample(*ec.table("uniform_water"))
        for speed in (0.0, -1500.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="uniform sound speed"):
                c.eikonal_solve(k["origin"], k["h"], k["n"], speed, k["src"])
        bad = np.full(k["n"], 1500.0, dtype=np.float32); bad[3, 4, 5] = np.nan
        with pytest.raises(ValueError, match="sound speed must be finite"):
            c.eikonal_solve(k["origin"], k["h"], k["n"], bad, k["src"])
        with pytest.raises(ValueError, match="must be"):
            c.eikonal_solve(k["origin"], k["h"], k["n"], bad[:-1], k["src"])
        for a in range(3):
            for off in (-0.01, k["n"][a] - 1 + 0.01):
                src = np.array(k["src"]); src[a] = k["origin"][a] + off * k["h"][a]
                with pytest.raises(ValueError, match="outside the grid"):
                    c.eikonal_solve(k["origin"], k["h"], k["n"], 1500.0, src)
        with pytest.raises(ValueError, match="init_radius"):
            c.eikonal_solve(k["origin"], k["h"], k["n"], 1500.0, k["src"], init_radius=0.99)
        with pytest.raises(ValueError, match="max_sweeps"):
            c.eikonal_solve(k["origin"], k["h"], k["n"], 1500.0, k["src"], max_sweeps=0)
        with pytest.raises(ValueError, match="too large"):
            c.eikonal_solve(k["origin"], k["h"], (2048, 1024, 1024), 1500.0, k["src"])
        c.eikonal_solve(k["origin"], k["h"], k["n"], 1500.0, k["src"])
        vox = int(np.prod(k["n"]))
        with pytest.raises(ValueError, match="outside the grid"):
            c.eikonal_sample([0, 1], [vox], [1.0])
        with pytest.raises(ValueError, match="row\\[0\\]"):
            c.eikonal_sample([1, 1], [0], [1.0])
        with pytest.raises(ValueError, match="not monotone"):
            c.eikonal_sample([0, 2, 1], [0], [1.0])
        with pytest.raises(ValueError, match="weight must be finite"):
            c.eikonal_sample([0, 1], [0], [np.nan])
        assert c.eikonal_sample([0, 0, 1], [5], [2.0])[0] == 0.0               # an empty row gives 0
        c.sync()
    finally:
        c.close()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_eikonal_delays_of_scene_a_end_to_end():
    sc, params, target, ref = ec.scene_a_method()
    arr = ec.array_of(sc["pos"])
    assert np.array_equal(arr.element_table()[0], sc["pos"])
    delays, info = Eikonal().solve(arr, target, params, return_volumes=True)
    dev = np.abs(delays[0] - ref["delays"]).max() * FREQ
    print(f"scene A end to end: largest |delays - oracle| = {dev:.3e} cycles, sweeps {info['sweeps']}")
    dev_e = np.abs(info["extra_path_m"][0] - ref["extra_path"]).max() * FREQ / sc["c_ref"]
    dev_t = np.abs(info["travel_time_s"][0] - ref["tau"]).max() * FREQ
    print(f"    extra path {dev_e:.3e} cycles, travel time {dev_t:.3e} cycles")
    assert delays.shape == (1, 9) and dev <= GATE_CYCLES and dev_e <= GATE_CYCLES and dev_t <= GATE_CYCLES
    assert np.abs(info["extra_path_m"][0]).max() * FREQ / sc["c_ref"] > 0.5          # the slab is worth more than half a cycle
    for got, want in zip(info["volumes"][0], (ref["T_med"], ref["T_ref"])):
        assert got.shape == sc["n"] and np.abs(got - want).max() <= GATE * want.max()
    assert all(1 <= s < 4 * sum(sc["n"]) for s in info["sweeps"][0])
    # calc_delays, a list of targets, and the Protocol seam give the same delays
    m = Eikonal()
    assert np.array_equal(m.calc_delays(arr, target, params), delays[0])
    assert np.array_equal(m.calc_delays(arr, [target, target], params), np.stack([delays[0], delays[0]]))
    d, a = ol.Protocol(delay_method=Eikonal(), apod_method=ol.apod_methods.Uniform()).beamform(arr, target, params)
    assert np.array_equal(d, delays[0]) and a.shape == (9,)
    # a transform: the array given in a shifted frame, moved back by M
    shift = np.array([0.3e-3, -0.2e-3, 0.05e-3])
    M = np.eye(4); M[:3, 3] = shift
    moved = ec.array_of(sc["pos"] - shift)
    dm = m.calc_delays(moved, target, params, transform=M)
    print(f"    with a transform: {np.abs(dm - ref['delays']).max() * FREQ:.3e} cycles")
    assert np.abs(dm - ref["delays"]).max() * FREQ <= GATE_CYCLES


@pytest.mark.gpu
def test_a_declared_uniform_medium_and_a_c_ref_volume():
    sc, params, target, ref = ec.scene_a_method()
    arr = ec.array_of(sc["pos"])
    direct = ol.get_engine().beamform(arr, target, sc["c_ref"])[0]
    declared = ec.Params(sc["n"], sc["origin"], sc["spacing"], sc["c_ref"], uniform_value=sc["c_ref"])
    d, info = Eikonal().solve(arr, target, declared)
    assert np.array_equal(d, direct) and info["sweeps"] == []                        # no solve: kernel 1's delays, bit for bit
    filled = ec.Params(np.full(sc["n"], sc["c_ref"], dtype=np.float32), sc["origin"], sc["spacing"], sc["c_ref"])
    d, info = Eikonal().solve(arr, target, filled)
    assert np.array_equal(info["extra_path_m"][0], np.zeros(9)) and info["sweeps"][0][0] == info["sweeps"][0][1]
    assert np.abs(d - direct).max() * FREQ <= 1e-9                                    # host fp64 against kernel 1's fp64


# ---- a solve changes nothing else -----------------------------------------------------------------------------------------------------
def _plain(a):
    return a.to_dict() if hasattr(a, "to_dict") else dict(vars(a))


def _same_analysis(a, b):
    """Two analyses of the same resident volumes.  The focal centroid is a quotient of fp64 sums that the scan adds up with one atomic per
    block, in whatever order the blocks finish, so two analyses of the SAME volumes may differ in its last bits: reordering n <= 2^15 terms
    moves sum p x / sum p by at most n 2^-53 max|x| = 2e-14 m = 2e-11 mm on this 6 mm scene.  Numbers therefore compare to 1e-10 (mm, and
    1e-12 relative); everything else, and the volumes the analysis is formed from, compares exactly."""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same_analysis(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same_analysis(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and isinstance(b, float):
        return math.isclose(a, b, rel_tol=1e-12, abs_tol=1e-10) or (math.isnan(a) and math.isnan(b))
    return a == b


@pytest.mark.gpu
def test_a_solve_leaves_the_other_resident_objects_untouched():
    arr = ol.Transducer.gen_matrix_array(nx=4, ny=4, pitch=2.1, kerf=0.2, units="mm", sensitivity=1e5)
    setup = ol.SimSetup(spacing=0.5, x_extent=(-6, 6), y_extent=(-6, 6), z_extent=(0, 16))
    mats = {"water": Material("water", 1500.0, 1000.0, 0.0022, 4182.0, 0.598), "skull": Material("skull", 2800.0, 1900.0, 6.0, 1300.0, 0.4)}
    proto = ol.Protocol(pulse=ol.Pulse(frequency=FREQ, duration=2e-5), sequence=ol.Sequence(pulse_interval=0.1, pulse_count=2, pulse_train_interval=1.0, pulse_train_count=1),
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
    before = (eng.ctx.field_fetch_all(), eng.ctx.thermal_fetch(), _plain(sol.analyze()))
    delays, info = Eikonal().solve(arr, ol.Point(position=(0, 0, 12), units="mm"), params)
    assert delays.shape == (1, 16) and np.abs(info["extra_path_m"][0]).max() > 0
    assert sol._device_is_current() and eng.ctx.field_variant() == variant
    after = (eng.ctx.field_fetch_all(), eng.ctx.thermal_fetch(), _plain(sol.analyze()))
    for key in ("pmag", "intensity"):
        assert np.array_equal(before[0][key], after[0][key]), key
    for a, b in zip(before[1], after[1]):
        assert np.array_equal(a, b)
    assert _same_analysis(before[2], after[2]), (before[2], after[2])
    eng.ctx.field_launch()          # the plan still launches, to the same bits (the solution was scaled: compare unscaled launches)
    again = eng.ctx.field_fetch_all()
    eng.ctx.field_launch()
    assert np.array_equal(again["pmag"], eng.ctx.field_fetch_all()["pmag"])


# ---- the debug library --------------------------------------------------------------------------------------------------------------
def test_eikonal_bounds_tag_only_in_the_debug_library():
    prod = open(os.path.join(LIB, "libolx.so"), "rb").read()
    dbg = open(os.path.join(LIB, "libolx_dbg.so"), "rb").read()
    assert b"olx_dbg_bounds_eikonal" in dbg and b"olx_dbg_bounds_eikonal" not in prod


@pytest.mark.gpu
def test_eikonal_kernels_stay_inside_their_extents_in_the_debug_library():
    env = dict(os.environ, OLX_LIB_PATH=os.path.join(LIB, "libolx_dbg.so"))
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "from openlifu_amd import _native as nat\n"
            "import eikonal_cases as ec\n"
            "ctx = nat.Context(0)\n"
            "for name in sorted(ec.CASES):\n"
            "    dev = ec.deviations(ec.run_device(ctx, name), name)\n"
            "    assert max(dev.values()) <= %r, (name, dev)\n"
            "ctx.sync()\n"
            "print('eikonal debug cases ok')\n") % (os.path.join(ROOT, "tests"), os.path.join(ROOT, "openlifu-python_amd"), GATE)
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "eikonal debug cases ok" in tail, tail
