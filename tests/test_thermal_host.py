"""Thermal model, host side (no GPU): the pulse schedule, the time axis and its FTCS bound, the fp64 oracle of the discrete
scheme against known answers (tests/thermal_oracle.py), and every refusal of run_thermal_simulation, raised before any device
call (DESIGN.md section 2 "thermal model")."""
import numpy as np
import pytest

import openlifu_amd as ol
from openlifu_amd.sim import thermal as th
from openlifu_amd.sim import run_thermal_simulation
from openlifu_amd.util import dataset as ds
import thermal_oracle as to


def _seq(**kw):
    return ol.Sequence(**kw)


def _per_focus(row_ptr, focus, tau, F):
    out = np.zeros(F)
    np.add.at(out, focus, tau)
    return out


# ---- schedule ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 2, 3])
@pytest.mark.parametrize("count", [6, 7, 10])
def test_schedule_per_focus_on_time_matches_get_ita_counts(F, count):
    pulse = ol.Pulse(frequency=500e3, duration=2e-5)
    seq = _seq(pulse_interval=0.1, pulse_count=count, pulse_train_interval=2.0, pulse_train_count=3)
    dur = seq.get_sequence_duration()
    dt = 0.037
    n = int(np.ceil(dur / dt))
    row_ptr, focus, tau = th.thermal_schedule(pulse, seq, F, dur / n, n)
    assert row_ptr.shape == (n + 1,) and row_ptr[0] == 0 and np.all(np.diff(row_ptr) >= 0) and row_ptr[-1] == focus.size
    # get_ita's pulse counts per focus (plan/solution.py: pulse_seq = (arange(pulse_count) - 1) % F + 1), per train
    pulse_seq = (np.arange(count) - 1) % F + 1
    counts = np.array([np.sum(pulse_seq == i + 1) for i in range(F)])
    on = _per_focus(row_ptr, focus, tau, F)
    assert np.allclose(on, counts * seq.pulse_train_count * min(pulse.duration, seq.pulse_interval), rtol=1e-12, atol=0)
    # the total on-time over the sequence duration is the sequence duty cycle
    sol = ol.Solution(pulse=pulse, sequence=seq)
    assert np.isclose(tau.sum() / dur, sol.get_sequence_dutycycle(), rtol=1e-12)


def test_schedule_back_to_back_trains_and_long_pulses():
    pulse = ol.Pulse(frequency=500e3, duration=0.5)          # longer than the interval: min(duration, interval)
    seq = _seq(pulse_interval=0.2, pulse_count=4, pulse_train_interval=0, pulse_train_count=2)
    dur = seq.get_sequence_duration()
    assert dur == pytest.approx(1.6)
    row_ptr, focus, tau = th.thermal_schedule(pulse, seq, 1, 0.1, 16)
    assert np.allclose(np.diff(row_ptr), 1) and np.allclose(tau, 0.1, rtol=1e-12)          # always on
    assert np.isclose(tau.sum() / dur, ol.Solution(pulse=pulse, sequence=seq).get_sequence_dutycycle(), rtol=1e-12)


def test_schedule_splits_straddling_pulses_exactly():
    pulse = ol.Pulse(frequency=500e3, duration=0.3)
    seq = _seq(pulse_interval=1.0, pulse_count=2, pulse_train_interval=0, pulse_train_count=1)
    # pulse 0 at [0, 0.3), pulse 1 at [1.0, 1.3); dt = 0.25 -> pulse 0 is split 0.25 + 0.05, pulse 1 0.25 + 0.05 (steps 4, 5)
    row_ptr, focus, tau = th.thermal_schedule(pulse, seq, 2, 0.25, 8)
    rows = {n: list(zip(focus[row_ptr[n]:row_ptr[n + 1]], tau[row_ptr[n]:row_ptr[n + 1]])) for n in range(8)}
    assert [f for f, _ in rows[0]] == [1] and rows[0][0][1] == pytest.approx(0.25, rel=1e-14)
    assert [f for f, _ in rows[1]] == [1] and rows[1][0][1] == pytest.approx(0.05, rel=1e-12)
    assert [f for f, _ in rows[4]] == [0] and rows[4][0][1] == pytest.approx(0.25, rel=1e-14)
    assert [f for f, _ in rows[5]] == [0] and rows[5][0][1] == pytest.approx(0.05, rel=1e-12)
    assert all(not rows[n] for n in (2, 3, 6, 7))
    # a run shorter than the sequence drops what comes after it
    row_ptr, focus, tau = th.thermal_schedule(pulse, seq, 2, 0.1, 2)
    assert tau.sum() == pytest.approx(0.2, rel=1e-12)


# ---- time axis ----------------------------------------------------------------------------------------------------------------------
def _layered(shape, seed=3):
    rng = np.random.default_rng(seed)
    rho = rng.uniform(900, 2000, shape)
    cp = rng.uniform(1000, 4200, shape)
    kap = rng.uniform(0.2, 0.6, shape)
    return rho, cp, kap


def test_time_axis_default_and_bound_anisotropic_heterogeneous():
    shape, h = (7, 6, 5), np.array([0.5e-3, 0.3e-3, 0.8e-3])
    rho, cp, kap = _layered(shape)
    for w in (0.0, 3e4):
        ref = to.ftcs_bound(rho, cp, kap, h, shape, w)
        assert th.thermal_bound(h, shape, rho, cp, kap, w) == pytest.approx(ref, rel=1e-13)
        dt, n, dt_max = th.thermal_time_axis(h, shape, rho, cp, kap, duration=1.0, perfusion=w)
        assert dt_max == pytest.approx(ref, rel=1e-13)
        assert n == int(np.ceil(1.0 / (ref / 2) * (1 - 1e-12))) and dt == pytest.approx(1.0 / n, rel=1e-14) and dt <= ref / 2
    # uniform medium: 1 / (2 kappa sum 1/h^2 / (rho Cp))
    b = th.thermal_bound(h, shape, 1000.0, 4182.0, 0.598)
    assert b == pytest.approx(1000.0 * 4182.0 / (2 * 0.598 * np.sum(1 / h ** 2)), rel=1e-13)
    with pytest.raises(ValueError, match="stability bound"):
        th.thermal_time_axis(h, shape, rho, cp, kap, duration=1.0, dt=1.001 * to.ftcs_bound(rho, cp, kap, h, shape))
    dt, n, _ = th.thermal_time_axis(h, shape, rho, cp, kap, duration=1.0, t_end=3.0)
    assert n * dt == pytest.approx(3.0, rel=1e-14)


# ---- oracle known answers -----------------------------------------------------------------------------------------------------------
RHO, CP, KAP = 1000.0, 4182.0, 0.598


def _always_on(n_steps, dt):
    return np.arange(n_steps + 1, dtype=np.int32), np.zeros(n_steps, dtype=np.int32), np.full(n_steps, dt)


def test_oracle_gaussian_source_centre_rise():
    sigma, h = 1e-3, 0.25e-3
    n = 41
    x = (np.arange(n) - n // 2) * h
    r2 = x[:, None, None] ** 2 + x[None, :, None] ** 2 + x[None, None, :] ** 2
    q0 = 2e6                                           # W/m^3 at the centre
    alpha = 10.0                                       # Np/m: I = Q / (2 alpha 1e4)
    inten = (q0 * np.exp(-r2 / (2 * sigma ** 2)) / (2 * alpha * 1e4))[None]
    dt_max = to.ftcs_bound(RHO, CP, KAP, (h, h, h), r2.shape)
    t_end = 1.0
    n_steps = int(np.ceil(t_end / (dt_max / 2)))
    dt = t_end / n_steps
    rp, fo, ta = _always_on(n_steps, dt)
    _, _, _, t = to.run(RHO, CP, KAP, alpha, inten, (h, h, h), rp, fo, ta, dt, n_steps)
    D = KAP / (RHO * CP)
    tau = np.linspace(0, t_end, 20001)
    exact = q0 / (RHO * CP) * np.trapezoid((sigma ** 2 / (sigma ** 2 + 2 * D * tau)) ** 1.5, tau)
    assert t[n // 2, n // 2, n // 2] == pytest.approx(exact, rel=1e-2)
    assert np.abs(t[0]).max() < 1e-3 * t.max()          # far from the boundary


@pytest.mark.parametrize("temp", [45.0, 43.0, 40.0])
def test_oracle_constant_temperature_cem43(temp):
    inten = np.zeros((1, 5, 5, 5))
    n_steps, dt = 30, 2.0
    rp, fo, ta = _always_on(n_steps, dt)
    _, cem, _, _ = to.run(RHO, CP, KAP, 0.0, inten, (1e-3,) * 3, rp, fo, ta, dt, n_steps, baseline=temp)
    R = 0.5 if temp >= 43 else 0.25
    assert np.allclose(cem, n_steps * dt / 60.0 * R ** (43.0 - temp), rtol=1e-13)


def test_oracle_energy_balance():
    n, h = 21, 0.5e-3
    rho, cp, kap = _layered((n, n, n), seed=5)
    inten = np.zeros((2, n, n, n))
    inten[0, 10, 10, 10] = 50.0
    inten[1, 9:12, 10, 11] = 20.0
    alpha = np.full((n, n, n), 30.0)
    dt = 0.4 * to.ftcs_bound(rho, cp, kap, (h, h, h), (n, n, n))
    n_steps = 7                                          # FTCS moves heat one voxel per step: the boundary stays at exactly 0
    rp = np.array([0, 1, 3, 3, 4, 5, 6, 6], dtype=np.int32)
    fo = np.array([0, 0, 1, 1, 0, 1], dtype=np.int32)
    ta = np.array([dt, 0.3 * dt, 0.5 * dt, dt, 0.1 * dt, 0.7 * dt])
    _, _, _, t = to.run(rho, cp, kap, alpha, inten, (h, h, h), rp, fo, ta, dt, n_steps)
    edge = max(np.abs(t[[0, -1]]).max(), np.abs(t[:, [0, -1]]).max(), np.abs(t[:, :, [0, -1]]).max())
    assert edge <= 1e-12 * t.max()
    stored = np.sum(rho * cp * t) * h ** 3
    deposited = sum(ta[e] * np.sum(2 * alpha * 1e4 * inten[fo[e]]) for e in range(rp[-1])) * h ** 3
    assert stored == pytest.approx(deposited, rel=1e-9)


def test_oracle_perfusion_steady_state():
    n, h, w = 31, 1e-3, 2e5
    inten = np.full((1, n, n, n), 10.0)
    alpha = 5.0
    q = 2 * alpha * 1e4 * 10.0
    dt = 0.5 * to.ftcs_bound(RHO, CP, KAP, (h, h, h), (n, n, n), w)
    n_steps = int(np.ceil(8 * RHO * CP / w / dt))
    rp, fo, ta = _always_on(n_steps, dt)
    _, _, _, t = to.run(RHO, CP, KAP, alpha, inten, (h, h, h), rp, fo, ta, dt, n_steps, perfusion=w)
    assert t[n // 2, n // 2, n // 2] == pytest.approx(q / w, rel=1e-2)


# ---- refusals, before any device call -----------------------------------------------------------------------------------------------
def _scene(n=(6, 5, 4), spacing=1.0, seg=None):
    setup = ol.SimSetup(spacing=spacing, x_extent=(0, spacing * (n[0] - 1)), y_extent=(0, spacing * (n[1] - 1)),
                        z_extent=(10, 10 + spacing * (n[2] - 1)))
    return setup.setup_sim_scene(ol.seg.seg_methods.UniformWater() if seg is None else seg)


def _solution(params, n_vol=1, n_foci=1):
    coords = params.coords
    dims = ["focal_point_index"] + list(coords.keys() if not hasattr(coords, "dims") else coords.dims)
    shape = (n_vol,) + tuple(len(coords[d]) for d in dims[1:])
    c = {"focal_point_index": np.arange(n_vol)}
    c.update({d: coords[d] for d in dims[1:]})
    res = ds.make_dataset({k: ds.make_dataarray(np.ones(shape, dtype=np.float32), coords=c, dims=dims, name=k,
                                                attrs={"units": u})
                           for k, u in (("p_min", "Pa"), ("p_max", "Pa"), ("intensity", "W/cm^2"))})
    return ol.Solution(delays=np.zeros((n_foci, 4)), apodizations=np.ones((n_foci, 4)), foci=[ol.Point()] * n_foci,
                       pulse=ol.Pulse(frequency=500e3, duration=2e-5),
                       sequence=ol.Sequence(pulse_interval=0.1, pulse_count=10, pulse_train_interval=1.0, pulse_train_count=1),
                       simulation_result=res)


def test_refuses_mismatched_coords():
    params = _scene()
    sol = _solution(_scene(n=(6, 5, 5)))
    with pytest.raises(ValueError, match="params.coords"):
        run_thermal_simulation(params, sol)
    with pytest.raises(ValueError, match="params.coords"):
        run_thermal_simulation(params, _solution(_scene(spacing=0.5)))


def test_refuses_dt_above_the_bound_and_negative_arguments():
    params = _scene()
    sol = _solution(params)
    bound = th.thermal_bound((1e-3,) * 3, (6, 5, 4), 1000.0, 4182.0, 0.598)
    with pytest.raises(ValueError, match="stability bound"):
        run_thermal_simulation(params, sol, dt=1.01 * bound)
    with pytest.raises(ValueError, match="t_end"):
        run_thermal_simulation(params, sol, t_end=-1.0)
    with pytest.raises(ValueError, match="perfusion"):
        run_thermal_simulation(params, sol, perfusion=-1.0)


@pytest.mark.parametrize("key", ["specific_heat", "thermal_conductivity"])
def test_refuses_missing_thermal_volumes(key):
    params = _scene()
    sol = _solution(params)
    reduced = ds.make_dataset({k: params[k] for k in params.data_vars if k != key} if hasattr(params, "data_vars")
                              else {k: params[k] for k in params.keys() if k != key})
    with pytest.raises(ValueError, match=key):
        run_thermal_simulation(reduced, sol)


def test_refuses_sharded_solution():
    params = _scene()
    with pytest.raises(NotImplementedError, match="thermal simulation: multi-GPU"):
        run_thermal_simulation(params, _solution(params, n_vol=1, n_foci=3))
