"""Pulse intensity integral and waveform traces of the pulsed model, host side: the fp64 oracle (tests/pulsed_wave_oracle.py) against
closed forms and against tests/pulsed_oracle.py, the refusals of run_simulation and run_thermal_simulation, and the ABI listing
(DESIGN.md section 2).  No GPU needed."""
import os
import re
import types

import numpy as np
import pytest

import openlifu_amd as ol
from openlifu_amd import _native as nat
from openlifu_amd.sim import field as sf
from openlifu_amd.sim import thermal as st
from openlifu_amd.util import dataset as ds
import pulsed_oracle as po
import pulsed_wave_oracle as pw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F0, C, RHO, P0 = 1e5, 1500.0, 1000.0, 1e5


# ---- 1. oracle known answer: one element, whole periods of K samples ---------------------------------------------------------------
@pytest.mark.parametrize("K", [8, 10, 16])
@pytest.mark.parametrize("cycles", [1, 5])
def test_oracle_single_element_pii_closed_form(K, cycles):
    dt = 1.0 / (K * F0)
    d, apod, area, alpha = 10.3 * C * dt, 0.7, 2e-6, 3.0          # arrival 10.3 samples after t = 0
    A = apod * area * P0 * F0 / C * np.exp(-alpha * d) / d
    T = cycles / F0
    args = ([[0.0, 0.0, d]], np.zeros((1, 3)), [area], [0.0], [apod], F0, C, RHO, P0, cycles, dt)
    pii, margin = pw.pulsed_pii(*args, 11 + cycles * K + 7, 1e-6, alpha)
    assert margin[0] > 0.2
    # sum of cos^2 over whole periods of K equidistant samples is K / 2 per period, and exactly cycles K samples are active
    assert pii[0] == pytest.approx(1e-4 * A * A * T / (2 * RHO * C), rel=1e-12)
    p, _ = pw.pulsed_waveforms(*args[:6], C, P0, cycles, dt, 11 + cycles * K + 7, 1e-6, alpha)
    assert np.count_nonzero(p[0]) == cycles * K and np.all(p[0][:11] == 0.0) and np.all(p[0][11 + cycles * K:] == 0.0)
    # n_t cuts the burst after m whole periods: the m-period value
    for m in range(cycles):
        cut, _ = pw.pulsed_pii(*args, 11 + m * K, 1e-6, alpha)
        assert cut[0] == pytest.approx(1e-4 * A * A * (m / F0) / (2 * RHO * C), rel=1e-12, abs=0.0 if m else 1e-300)


# ---- 2. oracle consistency: the peaks of the waveforms are the peaks of pulsed_oracle -----------------------------------------------
def test_waveform_peaks_equal_the_peak_oracle():
    n = 64
    pos = np.zeros((n, 3))
    pos[:, 0] = (np.arange(n) - (n - 1) / 2) * 0.5e-3
    area = np.full(n, 0.45e-3 * 10e-3)
    focus = np.array([1e-3, 0.0, 15e-3])
    delays = (np.linalg.norm(pos - focus, axis=1).max() - np.linalg.norm(pos - focus, axis=1)) / C
    apod = np.where(np.arange(n) % 9 == 0, 0.0, 1.0)             # (some elements off)
    rng = np.random.default_rng(11)
    pts = np.stack([rng.uniform(-8e-3, 8e-3, 200), rng.uniform(-3e-3, 3e-3, 200), rng.uniform(5e-3, 25e-3, 200)], axis=1)
    f0, dt, n_t, cycles, dmin, alpha = 400e3, 1.7e-7, 230, 3, 0.25e-3, 2.5
    p, margin = pw.pulsed_waveforms(pts, pos, area, delays, apod, f0, C, P0, cycles, dt, n_t, dmin, alpha)
    omax, omin, omargin = po.pulsed_points(pts, pos, area, delays, apod, f0, C, P0, cycles, dt, n_t, dmin, alpha)
    assert np.array_equal(margin, omargin)
    scale = max(omax.max(), omin.max())
    assert scale > 0
    assert np.abs(np.maximum(0.0, p.max(1)) - omax).max() <= 1e-12 * scale
    assert np.abs(np.maximum(0.0, -p.min(1)) - omin).max() <= 1e-12 * scale
    pii, _ = pw.pulsed_pii(pts, pos, area, delays, apod, f0, C, RHO, P0, cycles, dt, n_t, dmin, alpha)
    assert np.array_equal(pii, 1e-4 * dt / (RHO * C) * (p * p).sum(1))


# ---- 3. the continuous-wave model has neither ----------------------------------------------------------------------------------------
def _scene():
    arr = ol.Transducer.gen_matrix_array(nx=2, ny=2, pitch=4, kerf=0.4, units="mm", sensitivity=1e5)
    setup = ol.SimSetup(spacing=1.0, x_extent=(-2, 2), y_extent=(-2, 2), z_extent=(5, 9))
    return arr, setup.setup_sim_scene(ol.seg.seg_methods.UniformWater())


def test_cw_model_refuses_pii_and_record_points():
    arr, params = _scene()
    with pytest.raises(ValueError, match='field_model="pulsed"'):
        sf.run_simulation(arr, params, freq=400e3, field_model="cw", pulse_intensity_integral=True)
    with pytest.raises(ValueError, match='field_model="pulsed"'):
        sf.run_simulation(arr, params, freq=400e3, record_points=[[0, 0, 7]])


# ---- 4. run_thermal_simulation(pulse_energy=...) refusals ----------------------------------------------------------------------------
def _solution_stub(params, n_foci=2):
    """What run_thermal_simulation reads of a Solution before any device call."""
    coords = params.coords
    dims = list(coords.dims) if hasattr(coords, "dims") else list(coords.keys())
    shape = tuple(len(np.asarray(getattr(coords[d], "data", coords[d]))) for d in dims)
    c = {"focal_point_index": np.arange(n_foci)}
    c.update({d: coords[d] for d in dims})
    inten = ds.make_dataarray(np.ones((n_foci,) + shape, dtype=np.float32), coords=c, dims=["focal_point_index"] + dims, name="intensity")
    sol = types.SimpleNamespace(simulation_result={"intensity": inten}, num_foci=lambda: n_foci,
                                pulse=ol.Pulse(frequency=400e3, duration=2e-5),
                                sequence=ol.Sequence(pulse_interval=0.1, pulse_count=4, pulse_train_interval=0))
    return sol, shape


def test_thermal_refuses_bad_pulse_energy():
    _, params = _scene()
    sol, shape = _solution_stub(params)
    good = np.ones((2,) + shape)
    with pytest.raises(ValueError, match="pulse_energy must have shape"):
        st.run_thermal_simulation(params, sol, pulse_energy=good[:1])
    with pytest.raises(ValueError, match="pulse_energy must have shape"):
        st.run_thermal_simulation(params, sol, pulse_energy=good[:, :-1])
    bad = good.copy()
    bad[1, 0, 0, 0] = -1e-9
    with pytest.raises(ValueError, match="pulse_energy must be finite and >= 0"):
        st.run_thermal_simulation(params, sol, pulse_energy=bad)
    bad[1, 0, 0, 0] = np.nan
    with pytest.raises(ValueError, match="pulse_energy must be finite and >= 0"):
        st.run_thermal_simulation(params, sol, pulse_energy=bad)


# ---- 5. header and binding list the new names -------------------------------------------------------------------------------------------
def test_header_and_binding_list_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "olx.h")).read()
    assert re.search(r"#define\s+OLX_OUT_PII\s+128u", hdr)
    assert nat.OUT_PII == 128
    for name in ("olx_field_fetch_pii", "olx_field_pulse_trace"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in nat.SYMBOLS, name
    assert re.search(r"#define\s+OLX_ABI_VERSION\s+2\b", hdr)        # functions were only added
