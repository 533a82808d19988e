"""Impulse-response drive of the pulsed model, host side (no GPU): ``drive_taps`` against ``Transducer.calc_output``, the known answers of
the fp64 oracle (tests/pulsed_response_oracle.py), the option parsing and the refusals, and the conditions on the inputs of every GPU case of
tests/test_gpu_pulsed_response.py (arrival margins, tap conditioning)."""
import numpy as np
import pytest

import openlifu_amd as ol
from openlifu_amd.plan import protocol as pp
from openlifu_amd.sim import field as sf
import pulsed_response_cases as pc
import pulsed_response_oracle as pro
import pulsed_wave_oracle as pw

F0, C, RHO, P0 = pc.F0, pc.C, pc.RHO, pc.P0
DT = 1.0e-7
RESP_A = np.array([0.0, 0.6, 1.0, 0.3, -0.5, -0.2, 0.1])          # sampled at 2.5 DT: resampling to DT interpolates
RESP_E = np.array([1.0, -0.4, 0.2])
MARGIN, MAX_EXCLUDED = 1e-7, 1e-3


def small_array(**kw):
    return ol.Transducer.gen_matrix_array(nx=2, ny=2, pitch=3, kerf=0.3, units="mm", **kw)


def burst(cycles=3, dt=DT):
    n = int(round(cycles / (F0 * dt)))
    return np.sin(2 * np.pi * F0 * dt * np.arange(n))


def drive_from_taps(arr, g_of_e, delays, apod, signal, dt):
    """sum_m g_e[m] burst((k - m) dt) behind int(tau / dt) zeros, zero-padded to a common length."""
    rows = [np.concatenate([np.zeros(int(d / dt)), a * np.convolve(g, signal)]) for g, d, a in zip(g_of_e, delays, apod)]
    out = np.zeros((len(rows), max(len(r) for r in rows)))
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


# ---- drive_taps ------------------------------------------------------------------------------------------------------------------------
def test_no_response_gives_no_classes():
    cls, taps = sf.drive_taps(small_array(), DT)
    assert taps == [] and cls.shape == (4,) and cls.dtype == np.int32


def test_array_response_only():
    arr = small_array()
    arr.impulse_response, arr.impulse_dt = RESP_A, 2.5 * DT
    cls, taps = sf.drive_taps(arr, DT)
    assert np.array_equal(cls, np.zeros(4)) and len(taps) == 1
    assert np.array_equal(taps[0], arr.interp_impulse_response(DT)[0]) and len(taps[0]) == 16


def test_element_responses_only_group_into_classes():
    arr = small_array()
    for e in (1, 3):
        arr.elements[e].impulse_response, arr.elements[e].impulse_dt = RESP_E.copy(), DT
    cls, taps = sf.drive_taps(arr, DT)
    assert np.array_equal(cls, [0, 1, 0, 1]) and len(taps) == 2
    assert np.array_equal(taps[0], [1.0]) and np.array_equal(taps[1], RESP_E)


def test_both_responses_are_convolved_and_scalars_scale():
    arr = small_array()
    arr.impulse_response, arr.impulse_dt = RESP_A, 2.5 * DT
    arr.elements[1].impulse_response, arr.elements[1].impulse_dt = RESP_E.copy(), 2 * DT
    arr.elements[2].impulse_response = np.array([0.5])          # a length-1 response: a scalar, no impulse_dt
    cls, taps = sf.drive_taps(arr, DT)
    h = arr.interp_impulse_response(DT)[0]
    assert np.array_equal(cls, [0, 1, 2, 0])
    assert np.array_equal(taps[0], h)
    assert np.array_equal(taps[1], np.convolve(h, arr.elements[1].interp_impulse_response(DT)[0]))
    assert np.array_equal(taps[2], np.convolve(h, [0.5]))


def test_limits_name_themselves():
    arr = small_array()
    arr.impulse_response, arr.impulse_dt = np.ones(258), DT
    with pytest.raises(ValueError, match="256"):
        sf.drive_taps(arr, DT)
    arr.impulse_response, arr.impulse_dt = np.ones(256), DT
    assert len(sf.drive_taps(arr, DT)[1][0]) == 256
    arr = ol.Transducer.gen_matrix_array(nx=3, ny=2, pitch=3, kerf=0.3, units="mm")
    for e in range(5):
        arr.elements[e].impulse_response = np.array([1.0 + e])
    with pytest.raises(ValueError, match="4"):
        sf.drive_taps(arr, DT)
    arr.elements[4].impulse_response = np.array([1.0])
    assert len(sf.drive_taps(arr, DT)[1]) == 4


@pytest.mark.parametrize("which", ["array", "elements", "both"])
def test_calc_output_is_the_taps_applied_to_the_burst(which):
    arr = small_array()
    if which in ("array", "both"):
        arr.impulse_response, arr.impulse_dt = RESP_A, 2.5 * DT
    if which in ("elements", "both"):
        arr.elements[0].impulse_response, arr.elements[0].impulse_dt = RESP_E.copy(), 2 * DT
        arr.elements[3].impulse_response = np.array([-0.7])
    delays, apod = np.array([0.0, 3.4e-7, 1.25e-6, 9.9e-8]), np.array([1.0, 0.5, 0.0, 2.0])
    cls, taps = sf.drive_taps(arr, DT)
    ref = arr.calc_output(burst(), DT, delays=delays, apod=apod)
    mine = drive_from_taps(arr, [taps[c] for c in cls], delays, apod, burst(), DT)
    assert ref.shape == mine.shape
    assert np.allclose(ref, mine, rtol=0, atol=1e-14 * np.abs(ref).max())


# ---- the oracle's known answers -----------------------------------------------------------------------------------------------------
def _scene():
    k = pc.case("unit_tap")
    sel = np.random.default_rng(5).integers(0, len(k.pts), size=60)
    return k, k.pts[sel]


def test_oracle_unit_tap_is_the_plain_oracle():
    k, pts = _scene()
    p, m = pro.response_waveforms(pts, k.pos_m, k.area, k.delays[0], k.apod[0], k.cls, [np.array([1.0])], F0, C, P0, k.cycles, k.dt, k.n_t, k.dmin)
    q, mq = pw.pulsed_waveforms(pts, k.pos_m, k.area, k.delays[0], k.apod[0], F0, C, P0, k.cycles, k.dt, k.n_t, k.dmin)
    assert np.array_equal(m, mq) and np.abs(q).max() > 0
    assert np.abs(p - q).max() <= 1e-12 * np.abs(q).max()


def test_oracle_delayed_unit_tap_is_the_plain_oracle_three_steps_later():
    k, pts = _scene()
    p, _ = pro.response_waveforms(pts, k.pos_m, k.area, k.delays[0], k.apod[0], k.cls, [np.array([0.0, 0.0, 0.0, 1.0])], F0, C, P0, k.cycles, k.dt,
                                  k.n_t, k.dmin, absorption=3.0)
    later = (np.floor(k.delays[0] / k.dt) + 3.5) * k.dt          # every m_e + 3 (half a step inside: the floor is safe)
    q, _ = pw.pulsed_waveforms(pts, k.pos_m, k.area, later, k.apod[0], F0, C, P0, k.cycles, k.dt, k.n_t, k.dmin, absorption=3.0)
    assert np.abs(p - q).max() <= 1e-12 * np.abs(q).max()


def test_oracle_steady_state_amplitude_is_the_response_at_f0():
    g = pc.damped_sine(25, pc.DT0)
    pos, area = np.zeros((1, 3)), np.array([1e-6])
    pt = np.array([[0.3e-3, -0.2e-3, 9.1e-3]])
    d = np.linalg.norm(pt[0])
    p, _ = pro.response_waveforms(pt, pos, area, np.zeros(1), np.ones(1), np.zeros(1, int), [g], F0, C, P0, 40, pc.DT0, 700, 1e-4)
    u = d / C / pc.DT0
    steady = p[0, int(np.ceil(u)) + 24:int(np.ceil(u + 40 / (F0 * pc.DT0)))]          # every tap active
    assert len(steady) > 30 * 15
    H = abs((g * np.exp(-2j * np.pi * F0 * pc.DT0 * np.arange(25))).sum())
    amp = area[0] * P0 * F0 / C / d * H
    # 15 samples per period: the samples hit the crest to within cos(pi / 15)
    assert amp * np.cos(np.pi / 15) <= steady.max() <= amp * (1 + 1e-12) and amp * np.cos(np.pi / 15) <= -steady.min() <= amp * (1 + 1e-12)


# ---- options and refusals -------------------------------------------------------------------------------------------------------------
def test_drive_model_parsing():
    assert sf.parse_pulsed_drive_model(None) is None and sf.parse_pulsed_drive_model("") is None
    assert sf.parse_pulsed_drive_model(" Impulse_Response ") == "impulse_response"
    with pytest.raises(ValueError, match="drive_model"):
        sf.parse_pulsed_drive_model("fir")
    assert sf.parse_pulsed_drive_option({"field_model": "pulsed", "pulsed_drive_model": "impulse_response"}) == "impulse_response"
    assert sf.parse_pulsed_drive_option({"field_model": "pulsed"}) is None and sf.parse_pulsed_drive_option(None) is None
    with pytest.raises(ValueError, match="field_model"):
        sf.parse_pulsed_drive_option({"pulsed_drive_model": "impulse_response"})
    with pytest.raises(ValueError, match="drive_model"):
        sf.parse_pulsed_drive_option({"field_model": "pulsed", "pulsed_drive_model": "yes"})
    setup = ol.SimSetup(options={"field_model": "pulsed", "pulsed_drive_model": "impulse_response"})
    assert pp.pulsed_drive_from_options(setup) == "impulse_response"
    assert pp.pulsed_drive_from_options(ol.SimSetup()) is None


def test_refusals_without_and_with_the_opt_in():
    arr = small_array()
    arr.impulse_response, arr.impulse_dt = RESP_A, 2.5 * DT
    with pytest.raises(NotImplementedError, match="impulse_response"):
        sf.check_pulsed_supported(arr)
    sf.check_pulsed_supported(arr, False, "impulse_response")
    with pytest.raises(NotImplementedError, match="directivity"):
        sf.check_pulsed_supported(arr, True, "impulse_response")
    el = small_array()
    el.elements[2].impulse_response = np.array([0.5])
    with pytest.raises(NotImplementedError, match="element impulse_response"):
        sf.check_pulsed_supported(el)
    sf.check_pulsed_supported(el, drive_model="impulse_response")
    params = ol.SimSetup(spacing=1.0, x_extent=(-3, 3), y_extent=(-3, 3), z_extent=(4, 10)).setup_sim_scene(ol.seg.seg_methods.UniformWater())
    # refused before the engine (and a GPU) is asked for
    with pytest.raises(ValueError, match="drive_model"):
        sf.run_simulation(arr, params, freq=F0, field_model="cw", drive_model="impulse_response")
    with pytest.raises(ValueError, match="drive_model"):
        sf.run_simulation(arr, params, freq=F0, field_model="pulsed", drive_model="measured")
    with pytest.raises(ValueError, match="pulsed_drive_model"):
        sf.simulate_foci(arr, params, np.zeros((1, 4)), np.ones((1, 4)), F0, 1.0, pulsed_drive_model="impulse_response")
    with pytest.raises(NotImplementedError, match="impulse_response"):
        sf.run_simulation(arr, params, freq=F0, field_model="pulsed")
    hetero = ol.SimSetup(spacing=1.0, x_extent=(-3, 3), y_extent=(-3, 3), z_extent=(4, 10)).setup_sim_scene(ol.seg.seg_methods.UniformWater())
    speed = np.array(hetero["sound_speed"].data, dtype=np.float32)
    speed[:, :, 3] = 2800.0
    hetero["sound_speed"].data = speed
    for medium_model in (None, "straight_ray"):
        with pytest.raises(NotImplementedError, match="impulse_response"):
            sf.run_simulation(arr, hetero, freq=F0, field_model="pulsed", drive_model="impulse_response", medium_model=medium_model)


# ---- the inputs of the GPU cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_gpu_case_inputs(name):
    k = pc.case(name)
    assert k.conditioning() <= 4.0, f"sum |g| / |H(f0)| = {k.conditioning():.2f}"
    assert all(1 <= len(t) <= 256 for t in k.taps) and len(k.taps) <= 4
    for f in range(len(k.delays)):
        # (the margin is the plain model's: a property of the geometry, the steering and dt, not of the taps)
        _, margin = pw.pulsed_waveforms(k.pts, k.pos_m, k.area, k.delays[f], k.apod[f], F0, C, P0, k.cycles, k.dt, 1, k.dmin)
        share = (margin < MARGIN).mean()
        assert share <= MAX_EXCLUDED, f"focus {f}: {share:.2e} of the voxels within {MARGIN} of a sample"
