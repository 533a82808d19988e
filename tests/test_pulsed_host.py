"""Pulsed (tone-burst) field model, host side: the time axis, the delay truncation, the option parsing, the refusals and the fp64
oracle against hand-computed answers.  No GPU needed."""
import math

import numpy as np
import pytest

import openlifu_amd as ol
from openlifu_amd import dist
from openlifu_amd.plan.protocol import pulse_cycles, pulse_from_options
from openlifu_amd.sim import field as sf
from openlifu_amd.util import dataset as ds
import pulsed_oracle as po


# ---- 1. time axis -------------------------------------------------------------------------------------------------------------
def test_time_axis_given_dt_and_t_end():
    dt, n_t = sf.pulse_time_axis([1e-3] * 3, (10, 20, 30), dt=1e-7, t_end=2.05e-5, cfl=0.5)
    assert dt == 1e-7 and n_t == math.floor(2.05e-5 / 1e-7) + 1 == 206


def test_time_axis_defaults():
    sp, n = (2.5e-4, 5e-4, 1e-3), (256, 128, 64)
    dt, n_t = sf.pulse_time_axis(sp, n, dt=0, t_end=0, cfl=0.3)
    assert dt == 0.3 * 2.5e-4 / 1500.0
    t_end = math.sqrt((256 * 2.5e-4) ** 2 + (128 * 5e-4) ** 2 + (64 * 1e-3) ** 2) / 1500.0
    assert n_t == math.floor(t_end / dt) + 1
    # one default at a time
    assert sf.pulse_time_axis(sp, n, dt=1e-7, t_end=0)[1] == math.floor(t_end / 1e-7) + 1
    assert sf.pulse_time_axis(sp, n, dt=0, t_end=1e-5, cfl=0.5) == (0.5 * 2.5e-4 / 1500.0, math.floor(1e-5 / (0.5 * 2.5e-4 / 1500.0)) + 1)


def test_time_axis_rejects_negative_values():
    with pytest.raises(ValueError):
        sf.pulse_time_axis([1e-3] * 3, (4, 4, 4), dt=-1e-7)
    with pytest.raises(ValueError):
        sf.pulse_time_axis([1e-3] * 3, (4, 4, 4), t_end=-1.0)
    with pytest.raises(ValueError):
        sf.pulse_time_axis([1e-3] * 3, (4, 4, 4), dt=0, cfl=0)


# ---- 2. delay truncation --------------------------------------------------------------------------------------------------------
def test_delays_are_truncated_to_whole_steps():
    dt = 1e-7
    tau = np.array([0.0, 0.99e-7, 1.5e-7, 2.999e-7, 7.25e-7])
    assert np.array_equal(sf.truncate_delays(tau, dt), np.floor(tau / dt) * dt)
    assert np.allclose(sf.truncate_delays(tau, dt) / dt, [0, 0, 1, 2, 7])
    # the oracle's arrival steps start from the truncated delays: a delay and its half-step-shifted twin arrive together
    pos = np.array([[0.0, 0.0, 0.0], [1e-3, 0.0, 0.0]])
    pts = np.array([[0.0, 0.0, 0.02]])
    u1, _ = po.arrival_steps(pts, pos, tau[[2, 4]], dt, 1500.0, 1e-4)
    u2, _ = po.arrival_steps(pts, pos, (np.floor(tau[[2, 4]] / dt) + 0.5) * dt, dt, 1500.0, 1e-4)
    assert np.array_equal(u1, u2)


# ---- 3. option parsing ------------------------------------------------------------------------------------------------------------
def test_field_model_parsing():
    for v in (None, "", "cw", "CW", " cw "):
        assert sf.parse_field_model(v) == "cw"
    assert sf.parse_field_model("Pulsed") == "pulsed"
    with pytest.raises(ValueError):
        sf.parse_field_model("kwave")


def test_pulse_from_sim_setup_options():
    pulse = ol.Pulse(frequency=400e3, duration=2e-5)
    setup = ol.SimSetup(dt=1e-7, t_end=5e-5, cfl=0.4)
    assert pulse_from_options(setup, pulse) is None                 # absent: CW
    setup.options["field_model"] = "cw"
    assert pulse_from_options(setup, pulse) is None
    setup.options["field_model"] = "pulsed"
    assert pulse_from_options(setup, pulse) == (8.0, 1e-7, 5e-5, 0.4)
    # cycles as plan/protocol.py:223: min(round(duration f0), 20)
    assert pulse_cycles(ol.Pulse(frequency=400e3, duration=1e-3)) == 20.0
    assert pulse_cycles(ol.Pulse(frequency=500e3, duration=5e-6)) == 2.0
    setup.options["field_model"] = "tdfd"
    with pytest.raises(ValueError):
        pulse_from_options(setup, pulse)


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------
def _small_array():
    return ol.Transducer.gen_matrix_array(nx=2, ny=2, pitch=4, kerf=0.4, units="mm", sensitivity=1e5)


def test_pulsed_refuses_directivity_and_impulse_responses():
    arr = _small_array()
    with pytest.raises(NotImplementedError, match="directivity"):
        sf.check_pulsed_supported(arr, directivity=True)
    arr.elements[1].impulse_response = np.array([1.0])
    with pytest.raises(NotImplementedError, match="impulse_response"):
        sf.check_pulsed_supported(arr)
    arr = _small_array()
    arr.impulse_response = np.array([1.0])
    with pytest.raises(NotImplementedError, match="impulse_response"):
        sf.check_pulsed_supported(arr)
    sf.check_pulsed_supported(_small_array())          # plain array: accepted


def test_pulsed_refuses_a_heterogeneous_medium():
    setup = ol.SimSetup(spacing=1.0, x_extent=(-2, 2), y_extent=(-2, 2), z_extent=(5, 9))
    params = setup.setup_sim_scene(ol.seg.seg_methods.UniformWater())
    ss = params["sound_speed"]
    vol = np.full(ss.shape, 1500.0, dtype=np.float32)
    vol[:, :, 2:] = 2800.0
    params["sound_speed"] = ds.make_dataarray(vol, coords={d: ss.coords[d] for d in ss.dims}, dims=ss.dims, name="sound_speed",
                                              attrs=dict(ss.attrs))
    with pytest.raises(NotImplementedError, match="heterogeneous"):
        sf.run_simulation(_small_array(), params, freq=400e3, cycles=4, field_model="pulsed")
    with pytest.raises(ValueError):
        sf.run_simulation(_small_array(), params, freq=400e3, field_model="nonsense")


def test_pulsed_refuses_the_shard_paths():
    with pytest.raises(NotImplementedError, match="multi-GPU"):
        dist._continuous_wave_only(object(), (4.0, 1e-7, 0.0, 0.5))
    dist._continuous_wave_only(object(), None)          # CW: nothing to do


# ---- 5. the oracle against hand-computed answers ------------------------------------------------------------------------------------
F0, C = 1e5, 1500.0
DT = 1.0 / (8 * F0)              # 8 samples per period
W = 0.7 * 2e-6 * 1e5 * F0 / C    # apod * area * P0 * f0 / c


def _one_element(cycles, u, n_t=4096, delay=0.0, apod=0.7):
    """p_max, p_min of one element on axis whose arrival lies u samples after its (truncated) delay."""
    d = u * C * DT
    pos = np.zeros((1, 3))
    return po.pulsed_points([[0.0, 0.0, d]], pos, [2e-6], [delay], [apod], F0, C, 1e5, cycles, DT, n_t, 1e-6)[:2], d


def test_oracle_single_element_full_period():
    # arrival 10.25 samples after t = 0: the samples sit at phases (j + 0.75) / 8 of a period; the nearest to 0 and to 1/2 are 1/32 away
    (pmax, pmin), d = _one_element(cycles=2, u=10.25)
    a = W / d
    assert pmax[0] == pytest.approx(a * math.cos(math.pi / 16), rel=1e-12)
    assert pmin[0] == pytest.approx(a * math.cos(math.pi / 16), rel=1e-12)


def test_oracle_single_element_truncated_burst():
    # half a cycle = 4 samples k = 11 .. 14 at phases 0.75 / 8 .. 3.75 / 8 of a period
    (pmax, pmin), d = _one_element(cycles=0.5, u=10.25)
    a = W / d
    assert pmax[0] == pytest.approx(a * math.cos(2 * math.pi * 0.75 / 8), rel=1e-12)
    assert pmin[0] == pytest.approx(-a * math.cos(2 * math.pi * 3.75 / 8), rel=1e-12)
    # the time axis ends before the burst's negative half: nothing below zero was sampled
    (pmax, pmin), _ = _one_element(cycles=0.5, u=10.25, n_t=13)       # k = 11, 12 only
    assert pmax[0] == pytest.approx(a * math.cos(2 * math.pi * 0.75 / 8), rel=1e-12) and pmin[0] == 0.0
    # ... and before the arrival: nothing at all
    (pmax, pmin), _ = _one_element(cycles=0.5, u=10.25, n_t=11)
    assert pmax[0] == 0.0 and pmin[0] == 0.0


def test_oracle_separated_arrivals_never_add():
    # two elements at the same distance, the second delayed by 100 samples > T / dt = 16: p_max is the larger single peak, not the sum
    u = 10.25
    d = u * C * DT
    pos = np.zeros((2, 3))
    pts = [[0.0, 0.0, d]]
    both = po.pulsed_points(pts, pos, [2e-6, 2e-6], [0.0, 100 * DT], [0.7, 0.35], F0, C, 1e5, 2, DT, 4096, 1e-6)
    one = po.pulsed_points(pts, pos[:1], [2e-6], [0.0], [0.7], F0, C, 1e5, 2, DT, 4096, 1e-6)
    assert both[0][0] == one[0][0] == pytest.approx(W / d * math.cos(math.pi / 16), rel=1e-12)
    assert both[1][0] == one[1][0]
    # the same two elements delayed by 8 samples (one period) overlap: their terms add in phase
    near = po.pulsed_points(pts, pos, [2e-6, 2e-6], [0.0, 8 * DT], [0.7, 0.35], F0, C, 1e5, 2, DT, 4096, 1e-6)
    assert near[0][0] == pytest.approx(1.5 * W / d * math.cos(math.pi / 16), rel=1e-12)
