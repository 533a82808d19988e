"""Impulse-response and sampled drives of the full-wave model on the MI355X: fullwave_drive_k over the extended step range and
fullwave_drive_fir_k through the C-ABI (olx_fullwave_drive_response, olx_fullwave_drive_table, olx_fullwave_fetch_drive) against the fp64
oracles over the case table of tests/fullwave_drive_cases.py -- the drive table itself from the definition (tests/fullwave_drive_oracle.py),
the runs with the taps expanded into shifted entries (tests/fullwave_oracle.py, the split-layer and the lock-in oracle unchanged) -- then the
bit-identities, the state rules, the refusals, the debug library and run_fullwave_simulation / run_fullwave_steady_state end to end.

Gates:
  drive table   1e-12 |A_e| sum |g| per element: a ceiling -- the derived bound is about (M + 8) ulp, at most 6e-14 at M = 256
  runs          section 5.14's gate, 2e-5 of each record's maximum: the drive is fp64 on both sides, so nothing new enters it
  shift invariance on the device (the trace with the response vs. the fp64 FIR of the device's bare trace)   2e-5 of the maximum
  steady state  section 5.15's gate 5e-5 for the volume sums against the lock-in oracle of the expanded entries; against the known answer
                |G|, -arg G / 2 pi twice the deviation the fp64 oracle itself shows (tests/test_fullwave_drive_host.py)"""
import os
import subprocess
import sys
from ctypes import POINTER, c_int32

import numpy as np
import pytest

import openlifu_amd as ol
from openlifu_amd import _native as nat
from openlifu_amd.sim import field as sf
from openlifu_amd.sim import run_fullwave_simulation, run_fullwave_steady_state
import fullwave_cases as fc
import fullwave_drive_cases as dc
import fullwave_drive_oracle as do
import fullwave_lockin_oracle as lo
import fullwave_oracle as fo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "openlifu-python_amd", "lib")
GATE = 2e-5                  # section 5.14's
GATE_VOLUME = 5e-5           # section 5.15's
GATE_TABLE = 1e-12
FREQ = dc.FREQ


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


def table_deviation(got, name):
    """largest deviation of the drive table from the oracle's, per element as a fraction of |A_e| sum |g| (an element with A = 0 must be 0)"""
    k = dc.CASES[name]
    ref = dc.table(name)
    assert got.shape == ref.shape == (k["steps"], len(k["A"]))
    scale = np.abs(k["A"]) * dc.tap_norm(name)
    assert np.all(got[:, scale == 0] == 0.0)
    return float((np.abs(got - ref).max(axis=0)[scale > 0] / scale[scale > 0]).max())


# ---- 1. the drive table and the runs against the oracles ----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", dc.NAMES)
def test_drive_table_and_run_match_the_oracles(ctx, name):
    dc.set_sources(ctx, name)
    dev = table_deviation(ctx.fullwave_fetch_drive(), name)
    print(name, f"drive table {dev:.3e} of |A| sum |g|")
    assert dev <= GATE_TABLE
    check_gate(dc.run(ctx, name), dc.reference(name), name)


# ---- 2. bit identities --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_unit_taps_and_no_classes_are_the_bare_drive_to_the_bit(ctx):
    name = "f_identity"
    dc.set_sources(ctx, name, response=False)
    bare_table = ctx.fullwave_fetch_drive()
    bare = dc.run(ctx, name)
    check_gate(bare, dc.reference(name, False), "bare")
    dc.set_sources(ctx, name)                        # taps [1.0]
    assert np.array_equal(ctx.fullwave_fetch_drive(), bare_table)
    assert_same_bits(dc.run(ctx, name), bare)
    # a response, then n_classes = 0: the bare run of a context that never had one
    dc.set_sources(ctx, "a_one_class")
    assert not np.array_equal(ctx.fullwave_fetch_drive(), bare_table)
    ctx.fullwave_drive_response()
    assert np.array_equal(ctx.fullwave_fetch_drive(), bare_table)
    back = dc.run(ctx, "a_one_class")
    fresh = nat.Context(0)
    try:
        assert_same_bits(back, dc.run_device(fresh, "a_one_class", response=False))
    finally:
        fresh.close()
    assert_same_bits(back, bare)


@pytest.mark.gpu
def test_shift_invariance_on_the_device(ctx):
    name = "a_one_class"
    k = dc.CASES[name]
    bare = dc.run_device(ctx, name, response=False)[3].astype(np.float64)
    resp = dc.run_device(ctx, name)[3].astype(np.float64)
    want = do.fir(bare, k["taps"][0])
    dev = np.abs(resp - want).max() / np.abs(want).max()
    print(f"device trace vs the FIR of the device's bare trace: {dev:.3e}")
    assert dev <= GATE


@pytest.mark.gpu
def test_a_continued_run_equals_the_one_shot_run(ctx):
    one = dc.run_device(ctx, "b_layered")
    assert_same_bits(dc.run_device(ctx, "b_layered", split=137), one)
    assert_same_bits(dc.run_device(ctx, "g_split_layers", split=1), dc.run_device(ctx, "g_split_layers"))


# ---- 3. sampled tables --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_an_uploaded_table_reproduces_the_run_it_was_fetched_from(ctx):
    name = "b_layered"
    k = dc.CASES[name]
    dc.set_sources(ctx, name)
    tab = ctx.fullwave_fetch_drive()
    one = dc.run(ctx, name)
    dc.set_sources(ctx, name, response=False, A=np.ones(5), tau=np.zeros(5))          # another drive altogether, then the table
    ctx.fullwave_drive_table(tab)
    assert np.array_equal(ctx.fullwave_fetch_drive(), tab)
    assert_same_bits(dc.run(ctx, name), one)
    # the table is what is injected: minus the table, minus the field (p_max and p_min change places)
    ctx.fullwave_drive_table(-tab)
    neg = dc.run(ctx, name)
    assert np.array_equal(neg[0], one[1]) and np.array_equal(neg[1], one[0]) and np.array_equal(neg[2], one[2]) and np.array_equal(neg[3], -one[3])
    with pytest.raises(ValueError, match=r"shape \(400, 5\)"):
        ctx.fullwave_drive_table(tab[:-1])


# ---- 4. state -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_response_survives_a_new_drive_and_a_source_call_clears_it(ctx):
    name = "b_layered"
    k = dc.CASES[name]
    dc.set_sources(ctx, name, A=0.5 * k["A"] + 0.1, tau=k["tau_e"] + 1.3 * k["dt"])          # other (A, tau) first, with the response
    ctx.fullwave_drive(k["A"], k["tau_e"])
    assert table_deviation(ctx.fullwave_fetch_drive(), name) <= GATE_TABLE
    kept = dc.run(ctx, name)
    fresh = nat.Context(0)
    try:
        assert_same_bits(kept, dc.run_device(fresh, name))
    finally:
        fresh.close()
    dc.set_sources(ctx, name, response=False)          # the source call alone: the bare drive again
    bare = dc.run(ctx, name)
    check_gate(bare, dc.reference(name, False), "after a source call")
    assert not np.array_equal(bare[3], kept[3])
    # the drive calls reset the run
    dc.set_sources(ctx, name)
    ctx.fullwave_run(0, 5)
    ctx.fullwave_drive_response(k["cls"], k["taps"])
    with pytest.raises(nat.NativeError, match="does not continue"):
        ctx.fullwave_run(5, 2)
    ctx.fullwave_run(0, 5)
    ctx.fullwave_drive_table(np.zeros((k["steps"], 5)))
    with pytest.raises(nat.NativeError, match="does not continue"):
        ctx.fullwave_run(5, 2)


@pytest.mark.gpu
def test_calls_out_of_order_and_bad_arguments():
    c = nat.Context(0)
    ip = POINTER(c_int32)
    i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)

    def raw(n_classes, cls, row, taps):
        cls, row, taps = i32(cls), i32(row), np.ascontiguousarray(taps, dtype=np.float64)
        return c._lib.olx_fullwave_drive_response(c._h, n_classes, cls.ctypes.data_as(ip), row.ctypes.data_as(ip), nat._dptr(taps))

    try:
        out = np.zeros(20)
        for call in (lambda: c._lib.olx_fullwave_drive_response(c._h, 0, None, None, None), lambda: c._lib.olx_fullwave_drive_table(c._h, nat._dptr(out)),
                     lambda: c._lib.olx_fullwave_fetch_drive(c._h, nat._dptr(out))):
            assert call() == nat.OLX_ESTATE          # no plan
        c.fullwave_plan((0.5e-3,) * 3, (8, 8, 8), 1500.0, 1000.0, 0.0, 1500.0, 0, 0.0, 1e-7)
        c.fullwave_sources([5, 6], [1.0, 1.0], [0.0, 1e-7], FREQ, 3, 0, 10)          # the per-entry form has no drive table
        assert raw(1, [0, 0], [0, 1], [1.0]) == nat.OLX_ESTATE and "olx_fullwave_sources_elements as the last source call" in c._lib.olx_last_error(c._h).decode()
        assert c._lib.olx_fullwave_drive_table(c._h, nat._dptr(out)) == nat.OLX_ESTATE
        assert c._lib.olx_fullwave_fetch_drive(c._h, nat._dptr(out)) == nat.OLX_ESTATE
        for call in (lambda: c.fullwave_drive_response([0, 0], [[1.0]]), lambda: c.fullwave_drive_table(np.zeros((10, 2))), c.fullwave_fetch_drive):
            with pytest.raises(nat.NativeError, match="needs fullwave_sources_elements as the last source call"):
                call()          # the wrappers refuse before an array of unknown length goes to the library
        c.fullwave_sources_elements([5, 6], [0, 1], [1.0, 1.0], [1.0, 0.5], [0.0, 1e-7], FREQ, 3, 0, 10)
        bare = c.fullwave_fetch_drive()
        assert bare.shape == (10, 2)
        for args, what in (((1, [0, 1], [0, 1], [1.0]), "class 1 outside"), ((1, [-1, 0], [0, 1], [1.0]), "class -1 outside"),
                           ((1, [0, 0], [1, 2], [1.0, 1.0]), "must start at 0"), ((2, [0, 1], [0, 2, 2], [1.0, 1.0]), "class 1 has no taps"),
                           ((2, [0, 1], [0, 2, 1], [1.0, 1.0]), "strictly increasing"), ((1, [0, 0], [0, 257], np.ones(257)), "257 taps, at most"),
                           ((1, [0, 0], [0, 2], [1.0, np.nan]), "tap 1 is not finite"), ((1, [0, 0], [0, 2], [np.inf, 1.0]), "tap 0 is not finite"),
                           ((3, [0, 1], [0, 1, 2, 3], [1.0, 1.0, 1.0]), "3 classes for 2 elements"), ((-1, [0, 0], [0, 1], [1.0]), "-1 classes")):
            assert raw(*args) == nat.OLX_EINVAL, what
            assert what in c._lib.olx_last_error(c._h).decode(), (what, c._lib.olx_last_error(c._h).decode())
            assert np.array_equal(c.fullwave_fetch_drive(), bare)          # a refused call changes nothing
        assert c._lib.olx_fullwave_drive_response(c._h, 1, None, None, None) == nat.OLX_EINVAL
        assert raw(1, [0, 0], [0, 256], np.full(256, 1.0 / 256)) == 0          # 256 taps are taken
        with pytest.raises(ValueError, match="one entry per element"):
            c.fullwave_drive_response([0], [[1.0]])
        tab = np.zeros((10, 2)); tab[3, 1] = np.nan
        with pytest.raises(ValueError, match="step 3, element 1: the drive must be finite"):
            c.fullwave_drive_table(tab)
        assert c._lib.olx_fullwave_drive_table(c._h, None) == nat.OLX_EINVAL and c._lib.olx_fullwave_fetch_drive(c._h, None) == nat.OLX_EINVAL
        # a sampled table: A, tau and taps mean nothing to it until the next source call
        c.fullwave_drive_table(np.ones((10, 2)))
        with pytest.raises(nat.NativeError, match="olx_fullwave_drive: the drive table is a sampled one"):
            c.fullwave_drive([1.0, 1.0], [0.0, 0.0])
        with pytest.raises(nat.NativeError, match="olx_fullwave_drive_response: the drive table is a sampled one"):
            c.fullwave_drive_response([0, 0], [[1.0]])
        assert c._lib.olx_fullwave_drive_response(c._h, 0, None, None, None) == nat.OLX_ESTATE
        assert np.array_equal(c.fullwave_fetch_drive(), np.ones((10, 2)))
        c.fullwave_drive_table(np.full((10, 2), 2.0))          # another table is fine
        c.fullwave_sources_elements([5, 6], [0, 1], [1.0, 1.0], [1.0, 0.5], [0.0, 1e-7], FREQ, 3, 0, 10)
        assert np.array_equal(c.fullwave_fetch_drive(), bare)
        c.fullwave_drive_response([0, 1], [[0.5], [1.0, 1.0]])
        c.fullwave_drive([1.0, 0.5], [0.0, 1e-7])
        # olx_fullwave_layers and olx_fullwave_plan clear the sources, and the response with them
        c.fullwave_plan((0.5e-3,) * 3, (8, 8, 8), 1500.0, 1000.0, 0.0, 1500.0, 0, 0.0, 1e-7)
        assert raw(1, [0, 0], [0, 1], [1.0]) == nat.OLX_ESTATE
        with pytest.raises(nat.NativeError, match="needs fullwave_sources_elements as the last source call"):
            c.fullwave_fetch_drive()
        c.fullwave_sources_elements([5, 6], [0, 1], [1.0, 1.0], [1.0, 0.5], [0.0, 1e-7], FREQ, 3, 0, 10)
        assert np.array_equal(c.fullwave_fetch_drive(), bare)
        # the 2^28-byte limit applies to the extended table: 8192 elements x 4096 steps fill it exactly, one more tap is one row too many
        c.fullwave_sources_elements([5], [0], [1.0], np.ones(8192), np.zeros(8192), FREQ, 3, 0, 4096)
        with pytest.raises(ValueError, match=r"extended drive table of \(4096 \+ 1\) steps x 8192 elements"):
            c.fullwave_drive_response(np.zeros(8192, dtype=np.int32), [[0.5, 0.5]])
        c.fullwave_drive_response(np.zeros(8192, dtype=np.int32), [[0.5]])
        c.fullwave_run(0, 3)
        c.sync()
    finally:
        c.close()


# ---- 5. steady state ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_steady_state_carries_the_gain_of_the_response(ctx):
    got = dc.run_device_steady(ctx)
    C, S = dc.steady_reference(True)
    scale = np.hypot(C, S).max()
    dev = max(np.abs(got[0] - C).max(), np.abs(got[1] - S).max()) / scale
    print(f"steady state, volume sums vs the lock-in oracle of the expanded entries: {dev:.3e}")
    assert dev <= GATE_VOLUME
    bare = dc.run_device_steady(ctx, response=False)
    o_amp, o_ph = dc.known_answer_deviation(dc.steady_reference(False), (C, S))
    d_amp, d_ph = dc.known_answer_deviation(bare, got)
    print(f"known answer |G|, -arg G / 2 pi: device {d_amp:.3e}, {d_ph:.3e} cycles; fp64 oracle {o_amp:.3e}, {o_ph:.3e} cycles")
    assert d_amp <= 2 * o_amp and d_ph <= 2 * o_ph


# ---- 6. the debug library -----------------------------------------------------------------------------------------------------------------
def test_the_new_kernel_and_its_bounds_sites_are_in_both_libraries():
    prod = open(os.path.join(LIB, "libolx.so"), "rb").read()
    dbg = open(os.path.join(LIB, "libolx_dbg.so"), "rb").read()
    for kernel in (b"fullwave_drive_fir_k", b"fullwave_drive_k"):
        assert kernel in prod and kernel in dbg
    assert b"olx_dbg_bounds_fullwave" in dbg and b"olx_dbg_bounds_fullwave" not in prod


@pytest.mark.gpu
def test_drive_kernels_stay_inside_their_extents_in_the_debug_library():
    env = dict(os.environ, OLX_LIB_PATH=os.path.join(LIB, "libolx_dbg.so"))
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import numpy as np\n"
            "from openlifu_amd import _native as nat\n"
            "import fullwave_cases as fc, fullwave_drive_cases as dc\n"
            "ctx = nat.Context(0)\n"
            "for name in dc.NAMES:\n"
            "    k = dc.CASES[name]\n"
            "    dc.set_sources(ctx, name)\n"
            "    got, ref = ctx.fullwave_fetch_drive(), dc.table(name)\n"
            "    ctx.sync()\n"
            "    assert np.all(np.abs(got - ref).max(axis=0) <= %r * np.abs(k['A']) * dc.tap_norm(name)), name\n"
            "    dev = fc.deviations(dc.run(ctx, name), dc.reference(name))\n"
            "    assert max(dev.values()) <= %r, (name, dev)\n"
            "    ctx.sync()\n"
            "k = dc.CASES['b_layered']\n"
            "dc.set_sources(ctx, 'b_layered')\n"
            "ctx.fullwave_drive(0.5 * k['A'], k['tau_e'] - 2.5 * k['dt'])\n"
            "tab = ctx.fullwave_fetch_drive()\n"
            "ctx.fullwave_drive_response()\n"
            "dc.run(ctx, 'b_layered', split=137)\n"
            "dc.set_sources(ctx, 'b_layered', response=False)\n"
            "ctx.fullwave_drive_table(tab)\n"
            "dc.run(ctx, 'b_layered')\n"
            "dc.run_device_steady(ctx)\n"
            "ctx.sync()\n"
            "print('fullwave drive debug cases ok')\n") % (os.path.join(ROOT, "tests"), os.path.join(ROOT, "openlifu-python_amd"), GATE_TABLE, GATE)
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "fullwave drive debug cases ok" in tail, tail


# ---- 7. end to end ------------------------------------------------------------------------------------------------------------------------
PML = 6
RESP_A = np.array([0.1, 0.6, 1.0, -0.5, 0.2])
RESP_E = np.array([1.0, -0.4, 0.2])


def _product_scene():
    """case (a)'s three elements as the product sees them: the 20^3 interior of a 32^3 grid as ``params`` (mm, voxel 0 at 0), the array's
    response at the run's dt, element 1 with one more of its own -> (arr, params, n, h)"""
    n, h = (32, 32, 32), (0.5e-3,) * 3
    ext = (0.0, 19 * 0.5)
    setup = ol.SimSetup(spacing=0.5, x_extent=ext, y_extent=ext, z_extent=ext)
    params = setup.setup_sim_scene(ol.seg_methods.UniformWater())
    pos = [(9.3, 11.6, 8.25), (13.7, 10.4, 8.5), (11.5, 14.2, 9.75)]
    els = [ol.Element(index=e, position=(np.asarray(p) - PML) * 0.5, size=(0.4, 0.4), units="mm") for e, p in enumerate(pos)]
    arr = ol.Transducer(elements=els, frequency=FREQ, units="mm", sensitivity=1e5)
    arr.impulse_response, arr.impulse_dt = RESP_A.copy(), 1e-7
    arr.elements[1].impulse_response, arr.elements[1].impulse_dt = RESP_E.copy(), 1e-7
    return arr, params, n, h


def _entries(arr, n, h, A, tau, dt):
    """(ijk, amp, tau, element) of the point elements on the padded grid, from the oracle's rule"""
    pos = arr.element_table()[0]
    out = [[], [], [], []]
    for e in range(len(pos)):
        ijk, amp, tt = fo.monopole_entries(pos[e:e + 1], -PML * np.asarray(h), h, A[e:e + 1], tau[e:e + 1], 1500.0, FREQ, dt, n)
        for lst, v in zip(out, (ijk, amp, tt, np.full(len(amp), e))):
            lst.append(v)
    return tuple(np.concatenate(v) for v in out)


@pytest.mark.gpu
def test_run_fullwave_simulation_with_impulse_responses_and_with_sampled_waveforms_end_to_end():
    arr, params, n, h = _product_scene()
    delays, apod = np.array([0.2, 7.3, 3.4]) * 1e-7 + 0.37e-8, np.array([1.0, 0.7, 0.85])
    kw = dict(freq=FREQ, cycles=3, amplitude=2.0, pml_size=PML, ramp_cycles=1.0, pulse_intensity_integral=True, record_points=[[5.0, 5.0, 7.0]])
    out, raw = run_fullwave_simulation(arr, params, delays, apod, drive_model="impulse_response", **kw)
    dt, steps = raw["dt"], raw["n_steps"]
    cls, taps = sf.drive_taps(arr, dt)
    assert raw["drive_model"] == "impulse_response" and raw["drive_taps"] == 7 and [len(t) for t in taps] == [5, 7] and dt == pytest.approx(1e-7, rel=1e-12)
    A = apod * arr.element_table()[2] * 2.0 * 1e5 * FREQ / 1500.0
    base = _entries(arr, n, h, A, delays, dt)
    assert fo.activity_margin(base[2], 3.0 / FREQ, dt) >= 1e-6
    crop = (slice(PML, -PML),) * 3
    trace_ijk = [[10 + PML, 10 + PML, 14 + PML]]

    def check(out, raw, ref, what):
        for key in ("p_max", "p_min"):
            dev = np.abs(np.asarray(out[key].data) - ref[key][crop]).max() / ref[key][crop].max()
            print(what, key, f"{dev:.3e}")
            assert dev <= GATE
        assert np.abs(raw["p_trace"].T - ref["trace"]).max() <= GATE * np.abs(ref["trace"]).max()
        pii = 1e-4 * raw["dt"] * ref["psq"][crop] / (1000.0 * 1500.0)
        assert np.abs(np.asarray(out["pulse_intensity_integral"].data) - pii).max() <= GATE * pii.max()

    ijk, amp, tau = do.expand(base, cls, taps, dt)
    ref = fo.simulate(n, h, 1500.0, 1000.0, 0.0, 1500.0, PML, 2.0, dt, steps, ijk, amp, tau, FREQ, 3.0, 1.0, trace_ijk=trace_ijk)
    check(out, raw, ref, "impulse_response")
    # the default ignores the responses: the bare oracle, a shorter run
    out0, raw0 = run_fullwave_simulation(arr, params, delays, apod, **kw)
    assert raw0["drive_model"] is None and raw0["drive_taps"] is None and raw0["n_steps"] == steps - 6
    ref0 = fo.simulate(n, h, 1500.0, 1000.0, 0.0, 1500.0, PML, 2.0, dt, raw0["n_steps"], *base[:3], FREQ, 3.0, 1.0, trace_ijk=trace_ijk)
    check(out0, raw0, ref0, "default")
    assert not np.array_equal(np.asarray(out0["p_max"].data), np.asarray(out["p_max"].data))
    # sampled waveforms: the host-evaluated bare burst, in units of A_e, meets the same bare oracle
    W = np.stack([do.bare(np.arange(raw0["n_steps"]), 1.0, delays[e], FREQ, 3.0, 1.0, dt) for e in range(3)])
    kw_w = dict(kw, cycles=50, ramp_cycles=0.0)          # both are ignored
    outw, raww = run_fullwave_simulation(arr, params, None, apod, dt=dt, source_waveforms=W, **kw_w)
    assert raww["drive_model"] == "source_waveforms" and raww["n_steps"] == raw0["n_steps"] and raww["dt"] == dt
    check(outw, raww, ref0, "source_waveforms")


@pytest.mark.gpu
def test_run_fullwave_steady_state_with_impulse_responses_end_to_end():
    arr, params, n, h = _product_scene()
    delays, apod = np.array([0.2, 7.3, 3.4]) * 1e-7 + 0.37e-8, np.array([1.0, 0.7, 0.85])
    kw = dict(freq=FREQ, amplitude=2.0, pml_size=PML, lockin_cycles=4, settle_cycles=3, ramp_cycles=2.0)
    out, raw = run_fullwave_steady_state(arr, params, delays, apod, drive_model="impulse_response", **kw)
    dt, steps, (w0, nw) = raw["dt"], raw["n_steps"], raw["window"]
    cls, taps = sf.drive_taps(arr, dt)
    t_end = np.sqrt(3 * (20 * 0.5e-3) ** 2) / 1500.0 + delays.max() + 9.0 / FREQ + 6 * dt
    assert raw["drive_model"] == "impulse_response" and raw["drive_taps"] == 7 and steps == int(np.ceil(t_end / dt)) and raw["cycles"] == np.ceil(FREQ * t_end) + 1
    assert (w0, nw) == (steps - int(np.rint(4 / (FREQ * dt))), int(np.rint(4 / (FREQ * dt))))
    A = apod * arr.element_table()[2] * 2.0 * 1e5 * FREQ / 1500.0
    base = _entries(arr, n, h, A, delays, dt)
    assert fo.activity_margin(base[2], raw["cycles"] / FREQ, dt) >= 1e-6
    ijk, amp, tau = do.expand(base, cls, taps, dt)
    every = np.stack(np.meshgrid(*[np.arange(v) for v in n], indexing="ij"), axis=-1).reshape(-1, 3)
    tr = fo.simulate(n, h, 1500.0, 1000.0, 0.0, 1500.0, PML, 2.0, dt, steps, ijk, amp, tau, FREQ, raw["cycles"], 2.0, trace_ijk=every)["trace"]
    C, S = lo.volume_sums(tr, FREQ, dt, w0, nw)
    crop = (slice(PML, -PML),) * 3
    Aa, psi = lo.amplitude_phase(C.reshape(n)[crop], S.reshape(n)[crop], nw)
    got_A, got_psi = np.asarray(out["p_max"].data), np.asarray(out["phase"].data)
    dev_a = np.abs(got_A - Aa).max() / Aa.max()
    dev_p = np.abs(got_A * np.exp(2j * np.pi * got_psi) - Aa * np.exp(2j * np.pi * psi)).max() / Aa.max()
    print(f"steady state end to end: amplitude {dev_a:.3e}, amplitude x phase {dev_p:.3e} of the largest amplitude")
    # float32 outputs: half an ulp of the amplitude, and of the phase (at most 1/2 cycle) times 2 pi, on top of the sums' gate (section 5.15)
    assert dev_a <= GATE_VOLUME + 2.0 ** -24 and dev_p <= GATE_VOLUME + (1 + np.pi) * 2.0 ** -24
    # the default ignores the responses: a shorter run and another field
    out0, raw0 = run_fullwave_steady_state(arr, params, delays, apod, **kw)
    assert raw0["drive_model"] is None and raw0["drive_taps"] is None and raw0["n_steps"] == steps - 6
    assert not np.array_equal(np.asarray(out0["p_max"].data), got_A)
