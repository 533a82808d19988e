"""Impulse-response and sampled drives of the full-wave model without a GPU: the oracle's own identity (the taps expanded into shifted
entries = the FIR of the bare run's trace), ``drive_taps``'s keywords, every Python refusal before any device call, the growth of the run
by the longest response, what reaches the engine, and the three new C-ABI calls in the header and in the built library.

Measured with the fp64 oracle:
  expanded entries vs. the FIR of the bare trace, as a fraction of the trace maximum   1.2e-15 (a), 8.9e-16 (b)   gate 1e-12 (the element of (b) with tau < 0 enters through its expanded entries)
  steady state of tests/fullwave_drive_cases.py STEADY against the known answer |G|, -arg G / 2 pi: amplitude 1.19e-2 of |G|, phase 1.59e-3
  cycles (the lock-in's leakage over a window of 120 steps, and what is left of the transient)"""
import os
import re

import numpy as np
import pytest

import openlifu_amd as ol
from openlifu_amd import _native as nat
from openlifu_amd.sim import field as sf
from openlifu_amd.sim import fullwave as fw
from openlifu_amd.sim import run_fullwave_simulation, run_fullwave_steady_state
import fullwave_drive_cases as dc
import fullwave_drive_oracle as do
import fullwave_oracle as fo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F0 = 500e3
DT = 1.0e-7          # the default dt of the small scene: 0.3 x 0.5 mm / 1500 m/s
RESP_A = np.array([0.1, 0.6, 1.0, -0.5, 0.2])
RESP_E = np.array([1.0, -0.4, 0.2])
NEW_CALLS = ("olx_fullwave_drive_response", "olx_fullwave_drive_table", "olx_fullwave_fetch_drive")


def small_scene(response=True):
    arr = ol.Transducer.gen_matrix_array(nx=2, ny=2, pitch=1.0, kerf=0.1, units="mm", sensitivity=1e5)
    if response:
        arr.impulse_response, arr.impulse_dt = RESP_A.copy(), DT
        arr.elements[1].impulse_response, arr.elements[1].impulse_dt = RESP_E.copy(), DT
    setup = ol.SimSetup(spacing=0.5, x_extent=(-3, 3), y_extent=(-3, 3), z_extent=(0, 6))
    return arr, setup.setup_sim_scene(ol.seg_methods.UniformWater())


@pytest.fixture
def no_device(monkeypatch):
    """Any device call fails the test: what is refused must be refused on the host"""
    def boom(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(fw, "get_engine", boom)


class Stop(Exception):
    pass


@pytest.fixture
def seen(monkeypatch):
    """The engine replaced by one that records what ``fullwave`` / ``fullwave_steady`` are handed and stops there"""
    got = {}

    class Eng:
        def fullwave(self, spacing, npad, vols, c_ref, pml_size, pml_alpha, dt, n_steps, sources, freq, cycles, ramp, **kw):
            got.update(dt=dt, n_steps=n_steps, sources=sources, cycles=cycles, ramp=ramp)
            raise Stop

        def fullwave_steady(self, spacing, npad, vols, c_ref, pml_size, pml_alpha, dt, n_steps, sources, freq, cycles, ramp, **kw):
            got.update(dt=dt, n_steps=n_steps, sources=sources, cycles=cycles, ramp=ramp, window=kw["window"])
            raise Stop

    monkeypatch.setattr(fw, "get_engine", lambda: Eng())
    return got


# ---- the oracle's own identity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a_one_class", "b_layered"])
def test_expanded_entries_are_the_fir_of_the_bare_trace(name):
    k = dc.CASES[name]
    resp = dc.reference(name)["trace"]
    sim = lambda ijk, amp, tau: fo.simulate(k["n"], k["h"], k["c"], k["rho"], k["alpha"], k["c_ref"], k["pml"], k["pml_alpha"], k["dt"], k["steps"], ijk, amp, tau,
                                            k["freq"], k["cycles"], k["ramp"], trace_ijk=k["trace"])["trace"]
    amp, tau = k["amp1"] * k["A"][k["el"]], k["tau_e"][k["el"]]
    # The identity is one of runs that start at rest: the bare run of one class's elements at a time (the scheme is linear), each through its
    # own taps.  An element with tau < 0 (element 0 of case b) is outside it -- the part of its burst before step 0 is never injected, and each
    # tap cuts another part -- so its expanded entries, run on their own, join the sum as they are.
    early = tau < 0
    assert early.any() == (name == "b_layered")
    total = np.zeros(resp.shape)
    if early.any():
        total += sim(*do.expand((k["eijk"][early], amp[early], tau[early], k["el"][early]), k["cls"], k["taps"], k["dt"]))
    for c in range(len(k["taps"])):
        sel = np.isin(k["el"], np.flatnonzero(k["cls"] == c)) & ~early
        if sel.any():
            total += do.fir(sim(k["eijk"][sel], amp[sel], tau[sel]), k["taps"][c])
    dev = np.abs(total - resp).max() / np.abs(resp).max()
    print(name, f"identity {dev:.3e}")
    assert dev <= 1e-12


def test_oracle_table_with_unit_taps_is_the_bare_drive_and_a_delayed_tap_shifts_it():
    k = dc.CASES["b_layered"]
    one = [np.ones(1)] * 4
    s0 = do.drive_table(k["A"], k["tau_e"], k["cls"], one, k["freq"], k["cycles"], k["ramp"], k["dt"], k["steps"])
    for e in range(5):
        assert np.array_equal(s0[:, e], do.bare(np.arange(k["steps"]), k["A"][e], k["tau_e"][e], k["freq"], k["cycles"], k["ramp"], k["dt"]))
    assert s0[0, 0] != 0.0 and np.all(s0[:, 3] == 0.0)          # element 0 started before step 0; A = 0
    s3 = do.drive_table(k["A"], k["tau_e"], k["cls"], [np.array([0.0, 0.0, 0.0, 1.0])] * 4, k["freq"], k["cycles"], k["ramp"], k["dt"], k["steps"])
    assert np.array_equal(s3[3:], s0[:-3]) and s3[0, 0] == do.bare([-3], k["A"][0], k["tau_e"][0], k["freq"], k["cycles"], k["ramp"], k["dt"])[0] != 0.0


def test_oracle_steady_state_carries_the_gain_of_the_response():
    d_amp, d_ph = dc.known_answer_deviation(dc.steady_reference(False), dc.steady_reference(True))
    print(f"oracle steady state vs |G|: amplitude {d_amp:.3e}, phase {d_ph:.3e} cycles")
    assert d_amp <= 1.5 * 1.19e-2 and d_ph <= 1.5 * 1.59e-3          # the record plus half again


# ---- drive_taps ---------------------------------------------------------------------------------------------------------------------------
def test_drive_taps_defaults_are_the_pulsed_models():
    plain = ol.Transducer.gen_matrix_array(nx=2, ny=2, pitch=3, kerf=0.3, units="mm")
    cls, taps = sf.drive_taps(plain, DT)
    assert taps == [] and cls.shape == (4,) and cls.dtype == np.int32
    arr = ol.Transducer.gen_matrix_array(nx=2, ny=2, pitch=3, kerf=0.3, units="mm")
    arr.impulse_response, arr.impulse_dt = np.array([0.0, 0.6, 1.0, 0.3, -0.5, -0.2, 0.1]), 2.5 * DT
    arr.elements[1].impulse_response, arr.elements[1].impulse_dt = RESP_E.copy(), 2 * DT
    arr.elements[2].impulse_response = np.array([0.5])
    cls, taps = sf.drive_taps(arr, DT)
    h = arr.interp_impulse_response(DT)[0]
    assert np.array_equal(cls, [0, 1, 2, 0]) and np.array_equal(taps[0], h) and np.array_equal(taps[2], np.convolve(h, [0.5]))
    assert np.array_equal(taps[1], np.convolve(h, arr.elements[1].interp_impulse_response(DT)[0]))
    again = sf.drive_taps(arr, DT, max_classes=sf.PULSE_RESPONSE_MAX_CLASSES, max_taps=sf.PULSE_RESPONSE_MAX_TAPS, what="pulsed field model")
    assert np.array_equal(again[0], cls) and all(np.array_equal(a, b) for a, b in zip(again[1], taps))
    arr.impulse_response, arr.impulse_dt = np.ones(258), DT
    with pytest.raises(ValueError, match=re.escape("pulsed field model: element 0's impulse response has 258 taps at dt = 1e-07 s, at most 256 are supported")):
        sf.drive_taps(arr, DT)
    six = ol.Transducer.gen_matrix_array(nx=3, ny=2, pitch=3, kerf=0.3, units="mm")
    for e in range(5):
        six.elements[e].impulse_response = np.array([1.0 + e])
    with pytest.raises(ValueError, match=re.escape("pulsed field model: the elements carry more than 4 different impulse responses "
                                                   "(at most 4 classes of identical drive taps are supported)")):
        sf.drive_taps(six, DT)
    six.elements[4].impulse_response = np.array([1.0])
    assert len(sf.drive_taps(six, DT)[1]) == 4


def test_drive_taps_takes_a_class_per_element_for_the_full_wave_model():
    six = ol.Transducer.gen_matrix_array(nx=3, ny=2, pitch=3, kerf=0.3, units="mm")
    for e in range(6):
        six.elements[e].impulse_response = np.array([1.0 + e])
    cls, taps = sf.drive_taps(six, DT, max_classes=6, what="full-wave simulation")
    assert np.array_equal(cls, np.arange(6)) and [float(t[0]) for t in taps] == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]
    with pytest.raises(ValueError, match="full-wave simulation: the elements carry more than 5 different"):
        sf.drive_taps(six, DT, max_classes=5, what="full-wave simulation")
    with pytest.raises(ValueError, match="full-wave simulation: element 0's impulse response has 1 taps .* at most 0"):
        sf.drive_taps(six, DT, max_classes=6, max_taps=0, what="full-wave simulation")
    r = fw.response_of(six, DT)
    assert np.array_equal(r[0], np.arange(6)) and len(r[1]) == 6 and np.array_equal(r[2], np.ones(6))
    assert fw.response_of(ol.Transducer.gen_matrix_array(nx=3, ny=2, pitch=3, kerf=0.3, units="mm"), DT) is None
    six.impulse_response, six.impulse_dt = np.ones(257), DT
    with pytest.raises(ValueError, match="full-wave simulation: element 0's impulse response has 257 taps"):
        fw.response_of(six, DT)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_comes_before_any_device_call(no_device):
    arr, params = small_scene()
    W = np.zeros((4, 50))
    for bad in ("fir", "", "Impulse_Response", 1):
        with pytest.raises(ValueError, match="drive_model must be None or one of"):
            run_fullwave_simulation(arr, params, freq=F0, drive_model=bad)
        with pytest.raises(ValueError, match="drive_model must be None or one of"):
            run_fullwave_steady_state(arr, params, freq=F0, drive_model=bad)
        with pytest.raises(ValueError, match="drive_model must be None or one of"):
            fw.steady_state_run(params, np.zeros((1, 3)), [1.0], [0.0], F0, drive_model=bad)
    with pytest.raises(ValueError, match="needs the transducer"):
        fw.steady_state_run(params, np.zeros((1, 3)), [1.0], [0.0], F0, drive_model="impulse_response")
    with pytest.raises(ValueError, match="exclude each other"):
        run_fullwave_simulation(arr, params, freq=F0, dt=DT, source_waveforms=W, drive_model="impulse_response")
    with pytest.raises(ValueError, match="take no delays"):
        run_fullwave_simulation(arr, params, np.zeros(4), freq=F0, dt=DT, source_waveforms=W)
    for dt in (0, -1e-7, np.nan):
        with pytest.raises(ValueError, match="explicit dt > 0"):
            run_fullwave_simulation(arr, params, freq=F0, dt=dt, source_waveforms=W)
    for shape in ((3, 50), (4,), (4, 0), (1, 4, 50)):
        with pytest.raises(ValueError, match=r"source_waveforms must have shape \(4, n_t\)"):
            run_fullwave_simulation(arr, params, freq=F0, dt=DT, source_waveforms=np.zeros(shape))
    for bad in (np.nan, np.inf):
        Wb = W.copy(); Wb[2, 7] = bad
        with pytest.raises(ValueError, match="source_waveforms must be finite"):
            run_fullwave_simulation(arr, params, freq=F0, dt=DT, source_waveforms=Wb)
    with pytest.raises(ValueError, match="stability bound"):
        run_fullwave_simulation(arr, params, freq=F0, dt=1e-6, source_waveforms=W)
    arr.impulse_response, arr.impulse_dt = np.ones(300), DT          # 300 taps at the run's dt
    with pytest.raises(ValueError, match="full-wave simulation: element 0's impulse response has 3.. taps"):
        run_fullwave_simulation(arr, params, freq=F0, drive_model="impulse_response")
    with pytest.raises(ValueError, match="full-wave simulation: element 0's impulse response has 3.. taps"):
        run_fullwave_steady_state(arr, params, freq=F0, drive_model="impulse_response")
    assert "``impulse_response`` of the transducer and of its" in run_fullwave_simulation.__doc__          # ... is ignored by default: the docstring says so


def test_the_keywords_are_not_part_of_the_advertised_signatures():
    import inspect
    for fn, names in ((fw.run_fullwave_simulation, ("drive_model", "source_waveforms")), (fw.run_fullwave_steady_state, ("drive_model",))):
        for name in names:
            assert name not in inspect.signature(fn).parameters and fn.__kwdefaults__[name] is None and name in fn.__doc__


# ---- the run grows by the longest response; what reaches the engine -----------------------------------------------------------------------
DELAYS = np.array([0.0, 1e-6, 2e-6, 0.5e-6])
DIAG = np.sqrt(3 * (13 * 0.5e-3) ** 2) / 1500.0


def test_simulation_grows_by_each_elements_own_response(seen):
    arr, params = small_scene()
    with pytest.raises(Stop):
        run_fullwave_simulation(arr, params, DELAYS, freq=F0, cycles=3, pml_size=4)
    bare_steps = seen["n_steps"]
    assert isinstance(seen["sources"], tuple) and bare_steps == int(np.ceil((DIAG + 2e-6 + 3 / F0) / DT))          # the default ignores the responses
    with pytest.raises(Stop):
        run_fullwave_simulation(arr, params, DELAYS, freq=F0, cycles=3, pml_size=4, drive_model="impulse_response", apod=[1.0, 0.5, 0.0, 2.0])
    cls, taps = sf.drive_taps(arr, DT)
    assert [len(t) for t in taps] == [5, 7] and np.array_equal(cls, [0, 1, 0, 0])
    M = np.array([5, 7, 5, 5])
    assert seen["dt"] == pytest.approx(DT, rel=1e-14)
    assert seen["n_steps"] == int(np.ceil((DIAG + np.max(DELAYS + (M - 1) * seen["dt"]) + 3 / F0) / seen["dt"])) == bare_steps + 4
    src = seen["sources"]
    assert isinstance(src, dict) and np.array_equal(src["tau"], DELAYS) and np.array_equal(src["response"][0], cls)
    assert all(np.array_equal(a, b) for a, b in zip(src["response"][1], taps)) and "table" not in src
    area = arr.element_table()[2]
    assert np.allclose(src["A"], np.array([1.0, 0.5, 0.0, 2.0]) * area * 1e5 * F0 / 1500.0, rtol=1e-14, atol=0)
    # the entries carry A = 1: those of fw.monopole_table, with the element of each
    ijk, amp, _, el = fw.monopole_table(arr.element_table()[0], np.ones(4), DELAYS, [-3e-3, -3e-3, 0.0], 0.5e-3, (13, 13, 13), 1500.0, F0, seen["dt"])
    assert np.array_equal(src["elements"], el) and np.allclose(src["amplitude"], amp, rtol=1e-12, atol=0) and len(src["voxels"]) == len(el)
    # an explicit t_end is kept
    with pytest.raises(Stop):
        run_fullwave_simulation(arr, params, DELAYS, freq=F0, cycles=3, pml_size=4, t_end=200.5 * DT, drive_model="impulse_response")
    assert seen["n_steps"] == 201
    # a transducer without any response runs today's path
    plain, _ = small_scene(response=False)
    with pytest.raises(Stop):
        run_fullwave_simulation(plain, params, DELAYS, freq=F0, cycles=3, pml_size=4, drive_model="impulse_response")
    assert isinstance(seen["sources"], tuple) and seen["n_steps"] == bare_steps


def test_aperture_sources_take_the_response_as_they_are(seen):
    arr, params = small_scene()
    with pytest.raises(Stop):
        run_fullwave_simulation(arr, params, DELAYS, freq=F0, cycles=3, pml_size=4, element_model="aperture", drive_model="impulse_response")
    src = seen["sources"]
    assert set(src) == {"geometry", "A", "tau", "response"} and [len(t) for t in src["response"][1]] == [5, 7]


def test_steady_state_grows_by_the_longest_response(seen):
    arr, params = small_scene()
    kw = dict(freq=F0, pml_size=4, lockin_cycles=5, settle_cycles=2, ramp_cycles=1.5)
    with pytest.raises(Stop):
        run_fullwave_steady_state(arr, params, DELAYS, **kw)
    bare = dict(seen)
    t_end = DIAG + 2e-6 + 8.5 / F0
    assert bare["n_steps"] == int(np.ceil(t_end / DT)) and isinstance(bare["sources"], tuple)
    with pytest.raises(Stop):
        run_fullwave_steady_state(arr, params, DELAYS, drive_model="impulse_response", **kw)
    t_end += 6 * seen["dt"]
    assert seen["n_steps"] == int(np.ceil(t_end / seen["dt"])) == bare["n_steps"] + 6
    assert seen["cycles"] == np.ceil(F0 * t_end) + 1 and seen["cycles"] / F0 >= seen["n_steps"] * seen["dt"]
    nw = int(np.rint(5 / (F0 * seen["dt"])))
    assert seen["window"] == (seen["n_steps"] - nw, nw) and bare["window"] == (bare["n_steps"] - nw, nw)          # the window rule is unchanged
    src = seen["sources"]
    assert isinstance(src, dict) and [len(t) for t in src["response"][1]] == [5, 7] and np.array_equal(src["tau"], DELAYS)
    with pytest.raises(Stop):
        run_fullwave_steady_state(arr, params, DELAYS, drive_model="impulse_response", t_end=40e-6, **kw)
    assert seen["n_steps"] == 400


def test_source_waveforms_set_the_length_of_the_run(seen):
    arr, params = small_scene()
    W = np.arange(4 * 90, dtype=np.float64).reshape(4, 90) / 100.0
    with pytest.raises(Stop):
        run_fullwave_simulation(arr, params, None, [1.0, 0.5, 0.0, 2.0], freq=F0, dt=DT, source_waveforms=W, pml_size=4, cycles=50, ramp_cycles=7)
    src = seen["sources"]
    assert seen["n_steps"] == 90 and seen["dt"] == DT and src["table"].shape == (90, 4) and "response" not in src
    A = np.array([1.0, 0.5, 0.0, 2.0]) * arr.element_table()[2] * 1e5 * F0 / 1500.0
    assert np.array_equal(src["table"], (A[:, None] * W).T) and np.array_equal(src["tau"], np.zeros(4)) and seen["ramp"] == 0.0
    with pytest.raises(Stop):
        run_fullwave_simulation(arr, params, freq=F0, dt=DT, t_end=120.5 * DT, source_waveforms=W, pml_size=4)
    assert seen["n_steps"] == 121 and np.all(seen["sources"]["table"][90:] == 0.0) and np.array_equal(seen["sources"]["table"][:90, 1], W[1] * A[1] / 0.5)
    with pytest.raises(Stop):
        run_fullwave_simulation(arr, params, freq=F0, dt=DT, t_end=30 * DT, source_waveforms=W, pml_size=4)
    assert seen["n_steps"] == 90          # max(n_t, ceil(t_end / dt))


# ---- the C-ABI ----------------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_three_calls_and_the_library_exports_them():
    src = open(os.path.join(ROOT, "include", "olx.h")).read()
    assert "int olx_fullwave_drive_response(olx_ctx *ctx, int n_classes, const int32_t *class_of_element, const int32_t *row, const double *taps);" in src
    assert "int olx_fullwave_drive_table(olx_ctx *ctx, const double *table);" in src
    assert "int olx_fullwave_fetch_drive(olx_ctx *ctx, double *table);" in src
    lib = nat.load(require_gpu=False)
    for name in NEW_CALLS:
        assert name in nat.SYMBOLS and hasattr(lib, name)
    for so in ("libolx.so", "libolx_dbg.so"):
        blob = open(os.path.join(ROOT, "openlifu-python_amd", "lib", so), "rb").read()
        for name in NEW_CALLS + ("fullwave_drive_fir_k",):
            assert name.encode() in blob, (so, name)
