"""Rectangular element apertures of the full-wave model on the MI355X: fullwave_aperture_k, fullwave_drive_k and fullwave_inject_elem_k
through the C-ABI against the fp64 oracles (tests/fullwave_aperture_oracle.py for the weights, tests/fullwave_oracle.py for the runs) over
the case table of tests/fullwave_aperture_cases.py; the two inject forms against each other; bit-identical continued, repeated and
re-driven runs; the debug library; refusals; then run_fullwave_simulation, run_fullwave_steady_state and TimeReversal end to end.

Gates:
  weights   4 n_points 2^-53 of the element's largest weight: the summation bound of the definition, not a measurement
  runs      section 5.14's rule -- the largest deviation measured over the case table, as a fraction of each record's maximum, was
            1.50e-6 (the trace of the edges case; p_max / p_min <= 5.9e-7, sum p^2 <= 8.0e-7) <= 2.5e-6, so section 5.14's gate 2e-5 stays;
            the per-entry form and the element-factored form of one table gave the same bits on every case tried
  lock-in   section 5.15's gates for the volume and receiver sums of the steady state
  directivity scene (tests/test_fullwave_aperture_host.py)   <= 0.10 of the on-axis value at all six angles for the aperture model --
            twice the oracle's own deviation 0.052, fp32 against fp64 adds 1e-6 -- and >= 0.5 at 30 degrees for the point model
  TimeReversal with aperture receivers on the shrunken wedge scene (section 5.15's rule: eight times the measured value, rounded up to
            one digit): receiver sums measured 3.69e-7 of the largest |Z_e|, gate 3e-6; delays measured 2.70e-8 cycles, gate 3e-7"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import openlifu_amd as ol
from openlifu_amd import _native as nat
from openlifu_amd.seg.material import Material
from openlifu_amd.seg.seg_methods.threshold import SkullThreshold, skull_slab_image
from openlifu_amd.sim import run_fullwave_simulation, run_fullwave_steady_state, run_thermal_simulation
from openlifu_amd.sim import fullwave as fw
from openlifu_amd.util import dataset as ds
import fullwave_aperture_cases as ac
import fullwave_aperture_oracle as ao
import fullwave_cases as fc
import fullwave_lockin_cases as lc
import fullwave_lockin_oracle as lo
import fullwave_oracle as fo
import medium_delay_oracle as mo
import test_fullwave_aperture_host as host
import test_gpu_fullwave_lockin as lock_tests

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "openlifu-python_amd", "lib")
GATE = 2e-5                       # section 5.14's
GATE_VOLUME, GATE_RECEIVERS = 5e-5, 4e-5      # section 5.15's
GATE_TR_RECEIVERS, GATE_TR_DELAYS = 3e-6, 3e-7
FREQ = ac.FREQ
NAMES = sorted(ac.CASES)


@pytest.fixture(scope="module")
def ctx():
    c = nat.Context(0)
    yield c
    c.close()


def check_gate(got, ref, what=""):
    dev = fc.deviations(got, ref)
    print(what, {k: f"{v:.3e}" for k, v in dev.items()})
    for key, v in dev.items():
        assert v <= GATE, (what, key, v)


def assert_same_bits(a, b):
    for x, y in zip(a, b):
        assert (x is None and y is None) or np.array_equal(x, y)


# ---- 1. weights ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_weights_match_oracle(ctx, name):
    k = ac.CASES[name]
    row, vox, wt = ac.device_weights(ctx, name)
    o_row, o_ijk, o_wt = ac.weights(name)
    n_el = len(k["A"])
    assert row.shape == (n_el + 1,) and row[0] == 0 and row[-1] == vox.size == wt.size and wt.dtype == np.float64
    got = ao.dense(row, np.stack(np.unravel_index(vox, k["n"]), axis=1), wt, k["n"])
    ref = ao.dense(o_row, o_ijk, o_wt, k["n"])
    worst = 0.0
    for e in range(n_el):
        gate = 4 * int(k["nw"][e]) * int(k["nl"][e]) * 2.0 ** -53 * ref[e].max()
        worst = max(worst, np.abs(got[e] - ref[e]).max() / gate)
        assert np.abs(got[e] - ref[e]).max() <= gate, (name, e)
        assert abs(math.fsum(wt[row[e]:row[e + 1]]) - 1.0) <= gate, (name, e)
        assert np.all(np.diff(vox[row[e]:row[e + 1]]) > 0) and np.all(wt[row[e]:row[e + 1]] > 0)      # ascending voxels, no zero kept
    print(f"{name}: {vox.size} entries (oracle {o_wt.size}), largest deviation {worst:.3f} of the gate")


@pytest.mark.gpu
def test_a_capacity_that_is_too_small_reports_the_needed_size(ctx):
    full = ac.device_weights(ctx, "tilted")
    with pytest.raises(ValueError, match=f"{full[1].size} entries do not fit the capacity 10"):
        ac.device_weights(ctx, "tilted", capacity=10)
    assert_same_bits(full, ac.device_weights(ctx, "tilted", capacity=full[1].size))


# ---- 2. runs ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_runs_match_oracle(ctx, name):
    k = ac.CASES[name]
    assert fo.activity_margin(k["tau"], k["cycles"] / k["freq"], k["dt"]) >= 0.05 and 200 <= k["steps"] <= 400
    got = ac.run_device(ctx, name)
    ref = ac.reference(name)
    assert ref["p_max"].max() > 0 and ref["p_min"].max() > 0
    check_gate(got, ref, name)
    assert got[0].min() >= 0 and got[1].min() >= 0


# ---- 3. the two inject forms --------------------------------------------------------------------------------------------------------
def _close(a, b, what):
    for key, x, y in zip(("p_max", "p_min", "psq", "trace"), a, b):
        if x is None or x.size == 0:
            continue
        dev = np.abs(x.astype(np.float64) - y).max() / np.abs(y).max()
        print(what, key, f"{dev:.3e}")
        assert dev <= GATE, (what, key, dev)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tilted", "many_65"])
def test_per_entry_form_agrees_with_the_element_factored_form(ctx, name):
    _close(ac.run_device_entries(ctx, name), ac.run_device(ctx, name), name)


@pytest.mark.gpu
def test_one_point_apertures_agree_with_the_point_model(ctx):
    name = "many_65"
    k = ac.CASES[name]
    ijk, amp, tau = fo.monopole_entries(k["centre"], ac.ORIGIN, k["h"], k["A"], k["tau"], k["c"], k["freq"], k["dt"], k["n"])
    ac.plan(ctx, name)
    ctx.fullwave_sources(fc.lin(ijk, k["n"]), amp, tau, k["freq"], k["cycles"], k["ramp"], k["steps"], points=fc.lin(k["trace"], k["n"]))
    ctx.fullwave_run(0, k["steps"], psq=True)
    point = ctx.fullwave_fetch()
    _close(ac.run_device(ctx, name), point, "one point per element")


# ---- 4. bit-identical ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_continued_repeated_and_redriven_runs_are_bit_identical(ctx):
    one = ac.run_device(ctx, "tilted")
    assert_same_bits(one, ac.run_device(ctx, "tilted", split=137))
    assert_same_bits(one, ac.run_device(ctx, "tilted"))
    # olx_fullwave_drive with new (A, tau) over a resident table = a fresh olx_fullwave_sources_elements with the same values
    assert_same_bits(one, ac.run_device(ctx, "tilted", drive=True))
    k = ac.CASES["tilted"]
    A2, tau2 = k["A"][::-1].copy(), k["tau"] + 2.0 * k["dt"]
    fresh = ac.run_device(ctx, "tilted", A=A2, tau=tau2)
    ctx.fullwave_drive(k["A"], k["tau"])          # the table stays: only the drive changes, twice
    ctx.fullwave_drive(A2, tau2)
    ctx.fullwave_run(0, k["steps"], psq=True)
    assert_same_bits(fresh, ctx.fullwave_fetch())
    assert not np.array_equal(fresh[0], one[0])


@pytest.mark.gpu
def test_a_point_source_run_after_an_aperture_run_equals_a_fresh_context(ctx):
    ac.run_device(ctx, "axis_aligned")
    after = fc.run_device(ctx, "uniform_water")
    with pytest.raises(nat.NativeError, match="olx_fullwave_sources_elements as the last source call"):
        ctx.fullwave_drive(np.ones(4), np.zeros(4))
    fresh_ctx = nat.Context(0)
    try:
        fresh = fc.run_device(fresh_ctx, "uniform_water")
    finally:
        fresh_ctx.close()
    assert_same_bits(after, fresh)


# ---- 7. refusals at the C-ABI -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_calls_out_of_order_and_bad_arguments():
    c = nat.Context(0)
    try:
        k = ac.CASES["axis_aligned"]
        geom = (k["centre"], k["u"], k["v"], k["size"], k["nw"], k["nl"])
        with pytest.raises(nat.NativeError, match="olx_fullwave_apertures: no full-wave plan"):
            c.fullwave_apertures(*geom)
        with pytest.raises(nat.NativeError, match="olx_fullwave_sources_elements: no full-wave plan"):
            c.fullwave_sources_elements([0], [0], [1.0], [1.0], [0.0], FREQ, 3, 0, 10)
        ac.plan(c, "axis_aligned")
        with pytest.raises(nat.NativeError, match="olx_fullwave_drive: needs"):
            c.fullwave_drive([1.0], [0.0])
        vox = int(np.prod(k["n"]))
        for el in (-1, 2):
            with pytest.raises(ValueError, match=r"entry 1: element -?\d outside \[0, 2\)"):
                c.fullwave_sources_elements([5, 6], [0, el], [1.0, 1.0], [1.0, 1.0], [0.0, 0.0], FREQ, 3, 0, 10)
        with pytest.raises(ValueError, match="entry 0: amplitude must be finite"):
            c.fullwave_sources_elements([5], [0], [np.nan], [1.0], [0.0], FREQ, 3, 0, 10)
        with pytest.raises(ValueError, match="element 0: A and delay must be finite"):
            c.fullwave_sources_elements([5], [0], [1.0], [np.inf], [0.0], FREQ, 3, 0, 10)
        with pytest.raises(ValueError, match="outside the grid"):
            c.fullwave_sources_elements([vox], [0], [1.0], [1.0], [0.0], FREQ, 3, 0, 10)
        with pytest.raises(ValueError, match="drive table of 4097 steps x 8192 elements .* is too large"):
            c.fullwave_sources_elements([5], [0], [1.0], np.ones(8192), np.zeros(8192), FREQ, 3, 0, 4097)
        with pytest.raises(nat.NativeError, match="olx_fullwave_sources first"):      # none of the refused calls left a table
            c._fw_steps = 10
            c.fullwave_run(0, 10)
        bad = [np.array(a, dtype=np.float64, copy=True) if i < 4 else np.array(a, copy=True) for i, a in enumerate(geom)]
        bad[0][1, 2] = np.nan
        with pytest.raises(ValueError, match="element 1: centre, axes and size must be finite"):
            c.fullwave_apertures(*bad)
        bad[0][1, 2] = k["centre"][1, 2]; bad[4][2] = 0
        with pytest.raises(ValueError, match="element 2: n_w = 0"):
            c.fullwave_apertures(*bad)
        bad[4][2] = 300; bad[5][2] = 300
        with pytest.raises(ValueError, match="element 2: 90000 points are too many"):
            c.fullwave_apertures(*bad)
        bad[4][2], bad[5][2] = k["nw"][2], k["nl"][2]
        bad[0][3, 0] = 31.5 * k["h"][0]          # half a voxel beyond the last voxel of x
        with pytest.raises(ValueError, match="element 3 does not lie inside the grid"):
            c.fullwave_apertures(*bad)
        # a good table, then the drive's own refusals; the run still stands afterwards
        c.fullwave_sources_elements([5, 6], [0, 1], [1.0, 1.0], [1.0, 0.5], [0.0, 1e-7], FREQ, 3, 0, 10)
        with pytest.raises(ValueError, match="shape"):
            c.fullwave_drive([1.0], [0.0])
        with pytest.raises(ValueError, match="element 1: A and delay must be finite"):
            c.fullwave_drive([1.0, np.nan], [0.0, 0.0])
        c.fullwave_run(0, 4)
        c.fullwave_drive([1.0, 2.0], [0.0, 0.0])
        with pytest.raises(nat.NativeError, match="does not continue"):          # the drive reset the run
            c.fullwave_run(4, 2)
        c.fullwave_run(0, 10)
        c.sync()
    finally:
        c.close()


# ---- 6. the debug library -----------------------------------------------------------------------------------------------------------
def test_new_bounds_sites_only_in_the_debug_library():
    prod = open(os.path.join(LIB, "libolx.so"), "rb").read()
    dbg = open(os.path.join(LIB, "libolx_dbg.so"), "rb").read()
    for kernel in (b"fullwave_aperture_k", b"fullwave_drive_k", b"fullwave_inject_elem_k"):
        assert kernel in prod and kernel in dbg
    assert b"olx_dbg_bounds_fullwave" in dbg and b"olx_dbg_bounds_fullwave" not in prod


@pytest.mark.gpu
def test_aperture_kernels_stay_inside_their_extents_in_the_debug_library():
    env = dict(os.environ, OLX_LIB_PATH=os.path.join(LIB, "libolx_dbg.so"))
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import numpy as np\n"
            "from openlifu_amd import _native as nat\n"
            "import fullwave_cases as fc, fullwave_aperture_cases as ac, fullwave_aperture_oracle as ao\n"
            "ctx = nat.Context(0)\n"
            "for name in sorted(ac.CASES):\n"
            "    k = ac.CASES[name]\n"
            "    row, vox, wt = ac.device_weights(ctx, name)\n"
            "    ctx.sync()\n"
            "    got = ao.dense(row, np.stack(np.unravel_index(vox, k['n']), axis=1), wt, k['n'])\n"
            "    ref = ao.dense(*ac.weights(name), k['n'])\n"
            "    for e in range(len(k['A'])):\n"
            "        assert np.abs(got[e] - ref[e]).max() <= 4 * int(k['nw'][e]) * int(k['nl'][e]) * 2.0 ** -53 * ref[e].max(), (name, e)\n"
            "    dev = fc.deviations(ac.run_device(ctx, name), ac.reference(name))\n"
            "    assert max(dev.values()) <= %r, (name, dev)\n"
            "ac.run_device(ctx, 'tilted', split=137, drive=True)\n"
            "ctx.sync()\n"
            "print('fullwave aperture debug cases ok')\n") % (os.path.join(ROOT, "tests"), os.path.join(ROOT, "openlifu-python_amd"), GATE)
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "fullwave aperture debug cases ok" in tail, tail


# ---- 8. end to end ------------------------------------------------------------------------------------------------------------------
PML = 6


def _axis_aligned_product_scene():
    """The axis_aligned case as the product sees it: the 20^3 interior of its grid as ``params`` (mm, voxel 0 at 0), its elements as a
    Transducer -> (arr, params, case)"""
    k = ac.CASES["axis_aligned"]
    h_mm = k["h"][0] * 1e3
    ni = k["n"][0] - 2 * PML
    ext = (0.0, (ni - 1) * h_mm)
    setup = ol.SimSetup(spacing=h_mm, x_extent=ext, y_extent=ext, z_extent=ext)
    params = setup.setup_sim_scene(ol.seg_methods.UniformWater())
    assert np.asarray(params["sound_speed"].data).shape == (ni,) * 3 and float(params["sound_speed"].attrs["ref_value"]) == 1500.0
    els = [ol.Element(index=e, position=(k["centre"][e] - PML * np.array(k["h"])) * 1e3, size=k["size"][e] * 1e3, units="mm") for e in range(len(k["A"]))]
    return ol.Transducer(elements=els, frequency=FREQ, units="mm", sensitivity=1e5), params, k


def _oracle_entries(arr, k, A, tau, dt, rate=5):
    """The oracle's expanded entries of ``arr`` on the padded grid, formed here from the definition"""
    pos, _, area, _, _ = arr.element_table()
    size = np.array([[s * 1e-3 for s in el.size] for el in arr.elements])
    origin = -PML * np.array(k["h"])
    nw, nl = zip(*[ao.counts(s, k["h"], rate) for s in size])
    E = len(pos)
    row, ijk, wt = ao.aperture_table(pos, [host.EX] * E, [host.EY] * E, size, nw, nl, origin, k["h"], k["n"])
    return ao.expand(row, ijk, wt, A, tau, 1500.0, FREQ, dt, k["h"], k["n"]), (row, ijk, wt)


@pytest.mark.gpu
def test_aperture_table_on_the_callers_grid():
    arr, params, k = _axis_aligned_product_scene()
    ni = (k["n"][0] - 2 * PML,) * 3
    geom = fw.aperture_geometry(arr, k["h"], 5)
    row, ijk, wt = fw.aperture_table(geom, (0.0, 0.0, 0.0), k["h"], ni)
    o_row, o_ijk, o_wt = ao.aperture_table(geom["centre"], geom["u"], geom["v"], geom["size"], geom["n_w"], geom["n_l"], (0.0, 0.0, 0.0), k["h"], ni)
    assert np.array_equal(row, o_row) and np.array_equal(ijk, o_ijk) and ijk.dtype == np.int64
    for e in range(len(row) - 1):
        sl = slice(row[e], row[e + 1])
        assert np.abs(wt[sl] - o_wt[sl]).max() <= 4 * int(geom["n_w"][e]) * int(geom["n_l"][e]) * 2.0 ** -53 * o_wt[sl].max(), e
    assert np.array_equal(ijk[row[1]:row[2], 2], np.full(row[2] - row[1], 3))          # the element on a plane: voxel 9 of the padded grid


@pytest.mark.gpu
def test_run_fullwave_simulation_with_apertures_end_to_end():
    arr, params, k = _axis_aligned_product_scene()
    delays = np.array([0.2, 7.3, 3.4, 12.8]) * 1e-7 + 0.37e-8
    apod = np.array([1.0, 0.7, 0.0, 0.6])
    out, raw = run_fullwave_simulation(arr, params, delays, apod, freq=FREQ, cycles=3, amplitude=2.0, pml_size=PML, ramp_cycles=1.0,
                                       pulse_intensity_integral=True, record_points=[[5.0, 5.0, 7.0]], element_model="aperture", upsampling_rate=5)
    dt, steps = raw["dt"], raw["n_steps"]
    assert dt == pytest.approx(1e-7, rel=1e-12) and 150 <= steps <= 400
    area = arr.element_table()[2]
    A = apod * area * 2.0 * 1e5 * FREQ / 1500.0
    (ijk, amp, tau), table = _oracle_entries(arr, k, A, delays, dt)
    assert raw["element_model"] == "aperture" and raw["aperture_entries"] == table[2].size
    assert fo.activity_margin(tau, 3.0 / FREQ, dt) >= 1e-6
    ref = fo.simulate(k["n"], k["h"], 1500.0, 1000.0, 0.0, 1500.0, PML, 2.0, dt, steps, ijk, amp, tau, FREQ, 3.0, 1.0, trace_ijk=[[10 + PML, 10 + PML, 14 + PML]])
    crop = (slice(PML, -PML),) * 3
    pmax, pmin = np.asarray(out["p_max"].data), np.asarray(out["p_min"].data)
    for key, got in (("p_max", pmax), ("p_min", pmin)):
        dev = np.abs(got - ref[key][crop]).max() / ref[key][crop].max()
        print("end to end", key, f"{dev:.3e}")
        assert dev <= GATE
    assert np.abs(raw["p_trace"].T - ref["trace"]).max() <= GATE * np.abs(ref["trace"]).max()
    pii = 1e-4 * dt * ref["psq"][crop] / (1000.0 * 1500.0)
    assert np.abs(np.asarray(out["pulse_intensity_integral"].data) - pii).max() <= GATE * pii.max()
    # the default is the point model, to the same bits as before the argument existed
    a, ra = run_fullwave_simulation(arr, params, delays, apod, freq=FREQ, cycles=3, amplitude=2.0, pml_size=PML, ramp_cycles=1.0)
    b, rb = run_fullwave_simulation(arr, params, delays, apod, freq=FREQ, cycles=3, amplitude=2.0, pml_size=PML, ramp_cycles=1.0, element_model="point",
                                    upsampling_rate=3)
    assert ra["element_model"] == rb["element_model"] == "point" and ra["aperture_entries"] is None
    for key in ("p_max", "p_min", "intensity"):
        assert np.array_equal(np.asarray(a[key].data), np.asarray(b[key].data))
    assert not np.array_equal(np.asarray(a["p_max"].data), pmax)
    (p_ijk, p_amp, p_tau) = fo.monopole_entries(arr.element_table()[0], -PML * np.array(k["h"]), k["h"], A, delays, 1500.0, FREQ, dt, k["n"])
    refp = fo.simulate(k["n"], k["h"], 1500.0, 1000.0, 0.0, 1500.0, PML, 2.0, dt, steps, p_ijk, p_amp, p_tau, FREQ, 3.0, 1.0)
    assert np.abs(np.asarray(a["p_max"].data) - refp["p_max"][crop]).max() <= GATE * refp["p_max"][crop].max()


@pytest.mark.gpu
def test_steady_state_with_apertures_end_to_end():
    arr, params, k = _axis_aligned_product_scene()
    RAMP, SETTLE, LOCKIN = 1.0, 1.0, 3.0
    delays = np.array([0.2, 7.3, 3.4, 12.8]) * 1e-7 + 0.37e-8
    apod = np.array([1.0, 0.7, 0.0, 0.6])
    rec = np.array([[5.0, 5.0, 7.0], [2.3, 6.1, 4.2]])
    out, raw = run_fullwave_steady_state(arr, params, delays, apod, freq=FREQ, amplitude=2.0, lockin_cycles=LOCKIN, settle_cycles=SETTLE, ramp_cycles=RAMP,
                                         pml_size=PML, receivers=rec, element_model="aperture")
    dt, steps, (w0, nw), cycles = raw["dt"], raw["n_steps"], raw["window"], raw["cycles"]
    assert 150 <= steps <= 400 and raw["element_model"] == "aperture"
    A = apod * arr.element_table()[2] * 2.0 * 1e5 * FREQ / 1500.0
    src, table = _oracle_entries(arr, k, A, delays, dt)
    assert raw["aperture_entries"] == table[2].size
    every = np.stack(np.meshgrid(*[np.arange(v) for v in k["n"]], indexing="ij"), axis=-1).reshape(-1, 3)
    Zr, tr = lo.steady_receivers(k["n"], k["h"], 1500.0, 1000.0, 0.0, 1500.0, PML, 2.0, dt, steps, src, rec * 1e-3 + PML * np.array(k["h"]), FREQ, cycles, RAMP,
                                 w0, nw, trace_extra=every)
    C, S = lo.volume_sums(tr, FREQ, dt, w0, nw)
    crop = (slice(PML, -PML),) * 3
    Aref, psi = lo.amplitude_phase(C.reshape(k["n"])[crop], S.reshape(k["n"])[crop], nw)
    got_A, got_psi = np.asarray(out["p_max"].data), np.asarray(out["phase"].data)
    dev_a = np.abs(got_A - Aref).max() / Aref.max()
    dev_p = np.abs(got_A * np.exp(2j * np.pi * got_psi) - Aref * np.exp(2j * np.pi * psi)).max() / Aref.max()
    dev_r = np.abs(raw["receiver_sums"] - Zr).max() / np.abs(Zr).max()
    print(f"steady state with apertures: amplitude {dev_a:.3e}, amplitude x phase {dev_p:.3e}, receiver sums {dev_r:.3e}")
    assert dev_a <= GATE_VOLUME + 2.0 ** -24
    assert dev_p <= GATE_VOLUME + (1 + np.pi) * 2.0 ** -24
    assert dev_r <= GATE_RECEIVERS


def _scene_product(model):
    """The directivity scene of tests/test_fullwave_aperture_host.py through run_fullwave_steady_state -> amplitude [Pa per Pa m] at the six voxels"""
    s = host.SCENE
    h_mm = s["h"] * 1e3
    setup = ol.SimSetup(spacing=h_mm, x_extent=(0.0, (s["n"][0] - 1) * h_mm), y_extent=(0.0, (s["n"][1] - 1) * h_mm), z_extent=(0.0, (s["n"][2] - 1) * h_mm))
    params = setup.setup_sim_scene(ol.seg_methods.UniformWater())
    arr = ol.Transducer(elements=[ol.Element(position=np.array(s["centre"]) * h_mm, size=np.array(s["size"]) * 1e3, units="mm")], frequency=s["freq"], units="mm")
    dt = 0.3 * s["h"] / s["c"]
    out, raw = run_fullwave_steady_state(arr, params, freq=s["freq"], dt=dt, t_end=s["steps"] * dt, lockin_cycles=s["lock"], settle_cycles=1.0, ramp_cycles=s["ramp"],
                                         pml_size=s["pml"], element_model=model, upsampling_rate=s["rate"])
    assert raw["n_steps"] == s["steps"] and raw["aperture_entries"] == (78 if model == "aperture" else None)
    A0 = s["size"][0] * s["size"][1] * s["freq"] / s["c"]
    amp = np.asarray(out["p_max"].data, dtype=np.float64)
    return np.array([amp[tuple(p)] for p in host.scene_points()]) / A0


@pytest.mark.gpu
def test_directivity_scene_on_the_device():
    ref = host.scene_reference()
    dev = np.abs(_scene_product("aperture") - ref) / ref[0]
    print("directivity, aperture:", np.round(dev, 4))
    assert dev.max() <= 0.10
    devp = np.abs(_scene_product("point") - ref) / ref[0]
    print("directivity, point:", np.round(devp, 4))
    assert devp[3] >= 0.5


@pytest.mark.gpu
def test_time_reversal_with_aperture_receivers_matches_the_oracle():
    RAMP, SETTLE, LOCKIN = lock_tests.RAMP, lock_tests.SETTLE, lock_tests.LOCKIN
    arr, params, M, target, sc = lock_tests._wedge_product_scene()
    arr = ol.Transducer.gen_matrix_array(nx=4, ny=4, pitch=1.0, kerf=0.2, units="mm", sensitivity=1e5)          # 0.8 x 0.8 mm at the 1 mm pitch
    assert np.allclose([el.size for el in arr.elements], 0.8)
    axis = lock_tests._product_axis(sc)
    n_steps, cycles, w0, nw = axis
    q, h = sc["pml"], sc["h"]
    # the oracle: a unit monopole at the focus, the elements listen with their aperture averages
    size = np.full((16, 2), 0.8e-3)
    cn = ao.counts(size[0], h, 5)
    row, ijk, wt = ao.aperture_table(sc["pos"], [host.EX] * 16, [host.EY] * 16, size, [cn[0]] * 16, [cn[1]] * 16, (0, 0, 0), h, sc["n"])
    src = fo.monopole_entries(sc["focus"][None], (0, 0, 0), h, [1.0], [0.0], sc["c"], lc.F0, sc["dt"], sc["n"])
    uniq, inv = np.unique(ijk, axis=0, return_inverse=True)
    tr = fo.simulate(sc["n"], h, sc["c"], sc["rho"], sc["alpha"], lc.C0, q, 2.0, sc["dt"], n_steps, src[0], src[1], src[2], lc.F0, cycles, RAMP, trace_ijk=uniq)["trace"]
    inv = np.asarray(inv).reshape(-1)
    C, S = lo.receiver_sums(tr, {i: int(inv[i]) for i in range(len(ijk))}, row, np.arange(len(ijk)), wt, lc.F0, sc["dt"], w0, nw)
    Z = C + 1j * S
    crop = (slice(q, -q),) * 3
    ray = mo.delays(sc["pos"] - sc["shift"], (sc["focus"] - sc["shift"])[None], sc["c"][crop], -np.array([sc["half"], sc["half"], 0]) * h, (h,) * 3, lc.C0)[0]
    ref, margin, m, _ = lo.time_reversal(Z, ray, lc.F0)
    assert margin >= 0.25
    method = ol.delay_methods.TimeReversal(frequency=lc.F0, lockin_cycles=LOCKIN, settle_cycles=SETTLE, ramp_cycles=RAMP, pml_size=q, element_model="aperture")
    delays, amps, info = method.solve(arr, target, params, transform=M)
    raw = info["raw"][0]
    assert raw["n_steps"] == n_steps and raw["window"] == (w0, nw)
    dev_z = np.abs(raw["receiver_sums"] - Z).max() / np.abs(Z).max()
    dev = np.abs(delays[0] - ref).max() * lc.F0
    print(f"TimeReversal with aperture receivers: delays {dev:.3e} cycles, receiver sums {dev_z:.3e} of the largest, tie margin {info['tie_margin'][0]:.3f}")
    assert dev_z <= GATE_TR_RECEIVERS
    assert dev <= GATE_TR_DELAYS
    assert np.array_equal(info["cycles"][0], m)                          # the same whole cycles as the oracle
    point = ol.delay_methods.TimeReversal(frequency=lc.F0, lockin_cycles=LOCKIN, settle_cycles=SETTLE, ramp_cycles=RAMP, pml_size=q)
    _, amps_p, _ = point.solve(arr, target, params, transform=M)
    assert not np.allclose(amps[0], amps_p[0], rtol=1e-3)                # the average over 0.8 mm is not the sample at the centre
    proto = ol.Protocol(pulse=ol.Pulse(frequency=lc.F0, duration=2e-5),
                        delay_method=ol.delay_methods.TimeReversal(lockin_cycles=LOCKIN, settle_cycles=SETTLE, ramp_cycles=RAMP, pml_size=q, element_model="aperture"))
    d0, a0 = proto.beamform(arr, target, params)
    assert d0.shape == (16,) and d0.min() == 0.0 and np.isfinite(d0).all()


# ---- 5. an aperture run changes nothing else ----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_aperture_run_leaves_the_other_resident_objects_untouched():
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
    before = (eng.ctx.field_fetch_all(), eng.ctx.thermal_fetch(), sol.analyze())
    run_fullwave_simulation(arr, params, sol.delays[0], sol.apodizations[0], freq=FREQ, cycles=3, pml_size=PML, pulse_intensity_integral=True,
                            record_points=[[0.0, 0.0, 12.0]], element_model="aperture", upsampling_rate=2)
    assert sol._device_is_current() and eng.ctx.field_variant() == variant
    after = (eng.ctx.field_fetch_all(), eng.ctx.thermal_fetch(), sol.analyze())
    for key in ("pmag", "intensity"):
        assert np.array_equal(before[0][key], after[0][key]), key
    for a, b in zip(before[1], after[1]):
        assert np.array_equal(a, b)
    lock_tests._assert_same_analysis(before[2], after[2])
    eng.ctx.field_launch()
    again = eng.ctx.field_fetch_all()
    eng.ctx.field_launch()
    assert np.array_equal(again["pmag"], eng.ctx.field_fetch_all()["pmag"])
