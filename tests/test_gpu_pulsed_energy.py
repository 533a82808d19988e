"""Pulse intensity integral (OLX_OUT_PII) and waveform traces (olx_field_pulse_trace) of the pulsed model on the MI355X: kernel 2p's
<PII> and <TRACE> instantiations through the C-ABI against the fp64 oracle (tests/pulsed_wave_oracle.py), their agreement with each
other and with the peak volumes, the untouched default path, run_simulation's two arguments and run_thermal_simulation(pulse_energy=...).

Gates.  PII: max |PII_gpu - PII_oracle| <= 4e-5 of the oracle's volume maximum per focus -- the pressure gate is
1e-5 of the peak P, so |delta(p^2)| <= 2 |p| 1e-5 P, which summed over the n active samples against PII_max ~ n P^2 / 2 is at most 4e-5;
the fp32 sum of <= 1344 samples per lane and pass adds ~1e-6.  Traces: |trace - oracle| <= 1e-5 of the largest oracle sample.  Voxels
whose t_e / dt or (t_e + T) / dt lies within 1e-7 of an integer are excluded (fewer than 0.1 % of them), as in tests/test_gpu_pulsed.py,
whose four geometries, SHIFT and 60-cycle shape are copied here."""
import os
import subprocess
import sys

import numpy as np
import pytest

import openlifu_amd as ol
from openlifu_amd import _native as nat
from openlifu_amd.seg.material import Material
from openlifu_amd.sim import field as sf
from openlifu_amd.sim import run_thermal_simulation
from oracle import bf_oracle as bo
from conftest import centred_grid, synthetic_array
import pulsed_oracle as po
import pulsed_wave_oracle as pw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "openlifu-python_amd", "lib")
F0, C, RHO, P0 = 400e3, 1500.0, 1000.0, 1e5
PII_TOL, TRACE_TOL, MARGIN, MAX_EXCLUDED = 4e-5, 1e-5, 1e-7, 1e-3
SHIFT = np.array([0.0731, -0.0419, 0.0263]) * 1e-3          # (off the lattice of exact integer arrivals, as tests/test_gpu_pulsed.py)

CASES = {
    "linear64_1focus": dict(arr="linear", foci=[[0, 0, 15.0]], n=(32, 32, 32), h=0.5, cycles=3, t_end=0.0, absorption=0.0),
    "linear64_8foci_absorbing": dict(arr="linear", foci=[[x, 0, z] for x in (-3.0, 0.0, 3.0, 5.0) for z in (12.0, 18.0)], n=(32, 32, 32),
                                     h=0.5, cycles=4, t_end=4e-5, absorption=2.5),
    "matrix16x16_1focus": dict(arr="matrix", foci=[[0, 0, 25.0]], n=(32, 32, 32), h=1.0, cycles=3, t_end=5e-5, absorption=0.0),
    "matrix16x16_odd_absorbing": dict(arr="matrix", foci=[[2.0, -1.0, 20.0]], n=(33, 31, 35), h=1.0, cycles=5, t_end=0.0, absorption=5.0),
}


def linear_array(n=64, pitch_mm=0.5):
    pos = np.zeros((n, 3))
    pos[:, 0] = (np.arange(n) - (n - 1) / 2) * pitch_mm
    size = np.tile([0.9 * pitch_mm, 10.0], (n, 1))
    return pos, np.zeros_like(pos), size


def case_grid(k):
    nx, ny, nz = k["n"]
    xs = (np.arange(nx) - (nx - 1) / 2) * k["h"] * 1e-3 + SHIFT[0]
    ys = (np.arange(ny) - (ny - 1) / 2) * k["h"] * 1e-3 + SHIFT[1]
    zs = (5.0 + np.arange(nz) * k["h"]) * 1e-3 + SHIFT[2]
    return xs, ys, zs


def case_array(k):
    return linear_array() if k["arr"] == "linear" else synthetic_array(16, 16, 3.0)


def run_kernel(ctx, pos_mm, size, foci_mm, xs, ys, zs, cycles, dt=0.0, t_end=0.0, absorption=0.0, delays=None, apod=None, pii=True,
               launch=True, trace=None):
    """One pulsed plan with the oracle's steering -> (volumes dict | None, traces | None, setup dict).  ``pii``: plan with OUT_PII;
    ``trace``: linear voxel indices for olx_field_pulse_trace; ``launch=False``: the plan is traced without ever being launched."""
    pos_m = pos_mm * 1e-3
    area = size[:, 0] * size[:, 1] * 1e-6
    ctx.set_elements(pos_m, np.tile([0.0, 0.0, 1.0], (len(pos_m), 1)), area)
    if delays is None:
        steer = [bo.beamform(pos_m, np.zeros_like(pos_m), f, C) for f in np.atleast_2d(foci_mm) * 1e-3]
        delays, apod = np.array([s[0] for s in steer]), np.array([s[1] for s in steer])
    ctx.set_steering(delays, apod)
    sp = [xs[1] - xs[0], ys[1] - ys[0], zs[1] - zs[0]]
    n = (len(xs), len(ys), len(zs))
    dt, n_t = sf.pulse_time_axis(sp, n, dt, t_end, 0.5)
    ctx.field_absorption(absorption)
    ctx.field_pulse(cycles, dt, n_t)
    out = tr = None
    try:
        ctx.field_plan((xs[0], ys[0], zs[0]), sp, n, F0, C, RHO, P0,
                       flags=nat.OUT_PMAG | nat.OUT_INTENSITY | nat.OUT_PMAX | (nat.OUT_PII if pii else 0))
        if launch:
            ctx.field_launch()
            out = ctx.field_fetch_all(want=("pmag", "intensity", "pmax") + (("pii",) if pii else ()))
        if trace is not None:
            tr = ctx.field_pulse_trace(trace)
        ctx.sync()
    finally:
        ctx.field_pulse(0.0, 0.0, 0)
        ctx.field_absorption(0.0)
    X, Y, Z = np.meshgrid(xs, ys, zs, indexing="ij")
    setup = dict(delays=delays, apod=apod, area=area, pos_m=pos_m, dt=dt, n_t=n_t, cycles=cycles, absorption=absorption, dmin=0.5 * min(sp),
                 pts=np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1), shape=n)
    return out, tr, setup


def oracle_pii(s, f, sel=None):
    pts = s["pts"] if sel is None else s["pts"][sel]
    return pw.pulsed_pii(pts, s["pos_m"], s["area"], s["delays"][f], s["apod"][f], F0, C, RHO, P0, s["cycles"], s["dt"], s["n_t"], s["dmin"],
                         s["absorption"])


def oracle_traces(s, f, vox):
    return pw.pulsed_waveforms(s["pts"][vox], s["pos_m"], s["area"], s["delays"][f], s["apod"][f], F0, C, P0, s["cycles"], s["dt"], s["n_t"],
                               s["dmin"], s["absorption"])


def check_pii_gate(out, s, label):
    errs = []
    for f in range(len(s["delays"])):
        ref, margin = oracle_pii(s, f)
        ok = margin >= MARGIN
        assert (~ok).mean() < MAX_EXCLUDED, f"{(~ok).mean():.2e} of the voxels excluded"
        e = np.abs(out["pii"][f].ravel().astype(np.float64) - ref)[ok].max() / ref.max()
        print(f"[pii] {label} focus {f}: error {e:.3e} of the volume maximum {ref.max():.4e} J/cm^2, {(~ok).sum()} voxels excluded")
        errs.append(e)
    assert max(errs) <= PII_TOL, f"{label}: PII error {max(errs):.3e} of the volume maximum"
    return errs


def check_trace_gate(tr, s, vox, label):
    """Every sample of every kept point within TRACE_TOL of the largest oracle sample; exact zeros before the first arrival and from
    the last burst end on."""
    tdt = s["cycles"] / (F0 * s["dt"])
    for f in range(len(s["delays"])):
        ref, _ = oracle_traces(s, f, vox)
        e = np.abs(tr[f].astype(np.float64) - ref).max() / np.abs(ref).max()
        print(f"[trace] {label} focus {f}: error {e:.3e} of the largest sample {np.abs(ref).max():.4e} Pa over {len(vox)} points")
        assert e <= TRACE_TOL, f"{label} focus {f}: trace error {e:.3e}"
        live = s["apod"][f] != 0
        u, _ = po.arrival_steps(s["pts"][vox], s["pos_m"][live], s["delays"][f][live], s["dt"], C, s["dmin"])
        first, last = np.ceil(u.min(1)).astype(int), np.ceil((u + tdt).max(1)).astype(int)
        for i in range(len(vox)):
            assert np.all(tr[f, i, :max(first[i], 0)] == 0.0) and np.all(tr[f, i, max(last[i], 0):] == 0.0), (f, i)
        assert np.abs(tr[f]).max() > 0


@pytest.fixture(scope="module")
def ctx():
    c = nat.Context(0)
    yield c
    c.close()


# ---- 6. PII against the oracle, full volumes ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_pii_matches_oracle_small(ctx, name):
    """Measured on the MI355X (error of the volume maximum, worst focus): linear64_1focus 1.0e-6, linear64_8foci_absorbing 1.1e-6,
    matrix16x16_1focus 4.0e-7, matrix16x16_odd_absorbing 5.1e-7 (gate 4e-5); no voxel excluded."""
    k = CASES[name]
    pos, _, size = case_array(k)
    xs, ys, zs = case_grid(k)
    out, _, s = run_kernel(ctx, pos, size, k["foci"], xs, ys, zs, k["cycles"], t_end=k["t_end"], absorption=k["absorption"])
    check_pii_gate(out, s, name)


# ---- 7. single-element known answer on the device -----------------------------------------------------------------------------------
@pytest.mark.gpu
def test_pii_single_element_closed_form(ctx):
    K, cycles = 16, 5
    pos, size = np.zeros((1, 3)), np.array([[1.0, 1.0]])
    xs, ys, zs = centred_grid(24, 1.0)
    out, _, s = run_kernel(ctx, pos, size, None, xs, ys, zs, cycles, dt=1.0 / (K * F0), delays=np.zeros((1, 1)), apod=np.ones((1, 1)), absorption=4.0)
    u, d = po.arrival_steps(s["pts"], s["pos_m"], s["delays"][0], s["dt"], C, s["dmin"])
    whole = (np.ceil(u[:, 0] + cycles * K) <= s["n_t"])             # the burst ends inside the time axis
    assert 0.5 < whole.mean() < 1.0
    A = 1.0 * s["area"][0] * P0 * F0 / C * np.exp(-4.0 * d[:, 0]) / d[:, 0]
    want = 1e-4 * A * A * (cycles / F0) / (2 * RHO * C)
    got = out["pii"][0].ravel().astype(np.float64)
    e = np.abs(got - want)[whole].max() / want.max()
    print(f"[pii] single element: error {e:.3e} of the volume maximum")
    assert e <= PII_TOL
    assert np.all(got[~whole] < want[~whole] * (1 + 1e-5))           # a cut burst delivers less


# ---- 8. the default path is untouched -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["linear64_8foci_absorbing", "matrix16x16_odd_absorbing"])
def test_pii_flag_leaves_the_other_volumes_bit_equal(ctx, name):
    k = CASES[name]
    pos, _, size = case_array(k)
    xs, ys, zs = case_grid(k)
    a = run_kernel(ctx, pos, size, k["foci"], xs, ys, zs, k["cycles"], t_end=k["t_end"], absorption=k["absorption"], pii=True)[0]
    b = run_kernel(ctx, pos, size, k["foci"], xs, ys, zs, k["cycles"], t_end=k["t_end"], absorption=k["absorption"], pii=False)[0]
    assert "pii" in a and "pii" not in b
    for key in ("pmax", "pmag", "intensity"):
        assert np.array_equal(a[key], b[key]), key
    # without the flag there is nothing to fetch, and a continuous-wave plan refuses the flag
    with pytest.raises(nat.NativeError, match="OLX_OUT_PII"):
        ctx.field_fetch_all(want=("pii",))
    with pytest.raises(ValueError, match="OLX_OUT_PII needs a pulsed plan"):
        ctx.field_plan((xs[0], ys[0], zs[0]), [k["h"] * 1e-3] * 3, k["n"], F0, C, RHO, P0, flags=nat.OUT_PMAG | nat.OUT_PII)


# ---- 9 / 10. traces against the oracle, and against the volumes ---------------------------------------------------------------------------
def _trace_case(ctx):
    k = CASES["matrix16x16_1focus"]
    pos, _, size = case_array(k)
    xs, ys, zs = case_grid(k)
    foci = [k["foci"][0], [2.0, -1.0, 20.0]]                       # two foci in one plan
    n = k["n"]
    cand = np.random.default_rng(7).integers(0, n[0] * n[1] * n[2], size=64)
    fv = [int(np.argmin(np.abs(v - f * 1e-3))) for v, f in zip((xs, ys, zs), foci[0])]
    cand = np.append(cand, (fv[0] * n[1] + fv[1]) * n[2] + fv[2])       # ... and the focus voxel
    # the oracle's margin filter, over both foci (run once without a device result to learn the time axis)
    _, _, s = run_kernel(ctx, pos, size, foci, xs, ys, zs, k["cycles"], t_end=k["t_end"], launch=False)
    margin = np.minimum(*(oracle_traces(s, f, cand)[1] for f in range(2)))
    vox = cand[margin >= MARGIN]
    assert len(cand) - len(vox) <= 1, f"the margin filter dropped {len(cand) - len(vox)} of {len(cand)} candidates"
    return k, pos, size, foci, (xs, ys, zs), vox


@pytest.mark.gpu
def test_traces_match_oracle(ctx):
    """Measured on the MI355X: 2.7e-7 and 3.8e-7 of the largest sample for the two foci, 65 points (gate 1e-5)."""
    k, pos, size, foci, (xs, ys, zs), vox = _trace_case(ctx)
    # (the plan is traced without having been launched, and without OUT_PII)
    _, tr, s = run_kernel(ctx, pos, size, foci, xs, ys, zs, k["cycles"], t_end=k["t_end"], pii=False, launch=False, trace=vox)
    assert tr.shape == (2, len(vox), s["n_t"]) and tr.dtype == np.float32
    check_trace_gate(tr, s, vox, "matrix16x16 two foci")
    assert not np.array_equal(tr[0], tr[1])
    with pytest.raises(ValueError, match="outside the planned grid"):
        run_kernel(ctx, pos, size, foci, xs, ys, zs, k["cycles"], t_end=k["t_end"], launch=False, trace=[0, 32 * 32 * 32])
    with pytest.raises(nat.NativeError, match="needs a pulsed plan"):
        ctx.field_plan((xs[0], ys[0], zs[0]), [1e-3] * 3, k["n"], F0, C, RHO, P0, flags=nat.OUT_PMAG)
        ctx.field_pulse_trace([0])


@pytest.mark.gpu
def test_traces_agree_with_the_volumes(ctx):
    """Measured on the MI355X: the peaks of the traces are bit-equal to p_max / p_min at every traced voxel; PII from the traces
    (fp64 sum) agrees with the PII volume to 1.8e-7 relative."""
    k, pos, size, foci, (xs, ys, zs), vox = _trace_case(ctx)
    out, tr, s = run_kernel(ctx, pos, size, foci, xs, ys, zs, k["cycles"], t_end=k["t_end"], trace=vox)
    for f in range(2):
        t64 = tr[f].astype(np.float64)
        for key, peak in (("pmax", np.maximum(0.0, t64.max(1))), ("pmag", np.maximum(0.0, -t64.min(1)))):
            vol = out[key][f].ravel()
            e = np.abs(peak - vol[vox]).max() / vol.max()
            print(f"[trace] focus {f} {key}: {e:.3e} of the volume maximum, bit-equal: {np.array_equal(peak.astype(np.float32), vol[vox])}")
            assert e <= 1e-6, (f, key, e)
        pii_t = 1e-4 * s["dt"] / (RHO * C) * (t64 * t64).sum(1)
        pii_v = out["pii"][f].ravel()[vox].astype(np.float64)
        rel = np.abs(pii_t - pii_v) / pii_v
        print(f"[trace] focus {f} PII from the traces against the volume: {rel.max():.3e} relative")
        assert np.all(pii_v > 0) and rel.max() <= 1e-5, (f, rel.max())


@pytest.mark.gpu
def test_large_trace_takes_the_staged_fetch_and_agrees_with_the_volumes(ctx):
    """A trace of more than 8 MiB leaves the device through the staged fetch (worker threads on streams of their own): it must wait for
    the trace kernel.  8500 points x 2 foci x 151 samples = 10.3 MB; every point's peaks against the volumes of the same plan (gate 1e-6 of
    the volume maximum, as the 65-point test), a sample of rows against the oracle, and the call repeated gives the same array."""
    k, pos, size, foci, (xs, ys, zs), _ = _trace_case(ctx)
    vox = np.random.default_rng(8).integers(0, 32 ** 3, size=8500)
    out, tr, s = run_kernel(ctx, pos, size, foci, xs, ys, zs, k["cycles"], t_end=k["t_end"], trace=vox)
    assert tr.nbytes > 8 << 20
    for f in range(2):
        for key, peak in (("pmax", np.maximum(0.0, tr[f].max(1))), ("pmag", np.maximum(0.0, -tr[f].min(1)))):
            vol = out[key][f].ravel()
            e = np.abs(peak.astype(np.float64) - vol[vox]).max() / vol.max()
            print(f"[trace] 8500 points focus {f} {key}: {e:.3e} of the volume maximum")
            assert e <= 1e-6, (f, key, e)
    rows = np.r_[0:40, 4230:4270, 8460:8500]               # the start, the middle and the end of the transfer
    keep = rows[np.minimum(*(oracle_traces(s, f, vox[rows])[1] for f in range(2))) >= MARGIN]
    assert len(keep) >= len(rows) - 2
    check_trace_gate(tr[:, keep], s, vox[keep], "8500 points, 120 rows")
    again = run_kernel(ctx, pos, size, foci, xs, ys, zs, k["cycles"], t_end=k["t_end"], launch=False, trace=vox)[1]
    assert np.array_equal(tr, again)
    with pytest.raises(ValueError, match="OLX_PULSE_TRACE_MAX_SAMPLES"):
        run_kernel(ctx, pos, size, foci, xs, ys, zs, k["cycles"], t_end=k["t_end"], launch=False, trace=np.zeros(2 ** 18, dtype=np.int64))


@pytest.mark.gpu
def test_plan_keeps_its_own_time_step(ctx):
    """olx_field_pulse sets the model of the plans that FOLLOW: a call after the plan (another dt, or back to continuous wave) changes
    neither the launch nor the traces of the plan that exists."""
    k = CASES["matrix16x16_1focus"]
    pos, _, size = case_array(k)
    xs, ys, zs = case_grid(k)
    vox = np.array([5, 17000, 32767])
    out, tr, s = run_kernel(ctx, pos, size, k["foci"], xs, ys, zs, k["cycles"], t_end=k["t_end"], trace=vox)
    ctx.set_steering(s["delays"], s["apod"])
    ctx.field_pulse(k["cycles"], s["dt"], s["n_t"])
    sp = [xs[1] - xs[0], ys[1] - ys[0], zs[1] - zs[0]]
    ctx.field_plan((xs[0], ys[0], zs[0]), sp, k["n"], F0, C, RHO, P0, flags=nat.OUT_PMAG | nat.OUT_INTENSITY | nat.OUT_PMAX | nat.OUT_PII)
    for later in ((k["cycles"], 3.0 * s["dt"], s["n_t"]), (0.0, 0.0, 0)):
        ctx.field_pulse(*later)
        ctx.field_launch()
        got = ctx.field_fetch_all(want=("pmag", "intensity", "pmax", "pii"))
        for key in got:
            assert np.array_equal(got[key], out[key]), (later, key)
        assert np.array_equal(ctx.field_pulse_trace(vox), tr), later
    ctx.sync()


# ---- 11. a window longer than one LDS pass ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_pii_and_trace_window_longer_than_one_pass(ctx):
    """Measured on the MI355X: PII 4.3e-7 of the volume maximum, trace of the focus voxel 6.5e-7 of its largest sample."""
    pos, _, size = synthetic_array(4, 4, 3.0)
    xs, ys, zs = (v + s for v, s in zip(centred_grid(16, 1.0), SHIFT))
    dt = 1.0 / (40 * F0)                       # 40 samples per period, 60 cycles: T / dt = 2400 > 1344 samples per pass
    fv = [int(np.argmin(np.abs(v - f * 1e-3))) for v, f in zip((xs, ys, zs), (0.0, 0.0, 12.0))]
    vox = np.array([(fv[0] * 16 + fv[1]) * 16 + fv[2]])
    out, tr, s = run_kernel(ctx, pos, size, [[0, 0, 12.0]], xs, ys, zs, cycles=60, dt=dt, t_end=2e-4, trace=vox)
    assert 60 / (F0 * s["dt"]) > 64 * 21
    check_pii_gate(out, s, "60 cycles")
    assert oracle_traces(s, 0, vox)[1][0] >= MARGIN
    check_trace_gate(tr, s, vox, "60 cycles, focus voxel")


# ---- 12. public API -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_run_simulation_pii_and_record_points():
    arr = ol.Transducer.gen_matrix_array(nx=8, ny=8, pitch=4, kerf=0.4, units="mm", sensitivity=1e5)
    setup = ol.SimSetup(spacing=1.0, x_extent=(-10, 10), y_extent=(-10, 10), z_extent=(5, 35))
    params = setup.setup_sim_scene(ol.seg.seg_methods.UniformWater())
    kw = dict(freq=F0, cycles=6, dt=0, t_end=0, cfl=0.5, amplitude=1, field_model="pulsed")
    plain_ds, plain_raw = sf.run_simulation(arr, params, **kw)
    assert sorted(plain_ds.data_vars) == ["intensity", "p_max", "p_min"] and sorted(plain_raw) == ["backend", "p_max", "p_min"]
    ds_, raw = sf.run_simulation(arr, params, pulse_intensity_integral=True, record_points=[[0, 0, 30], [3, 0, 25]], **kw)
    shape = np.asarray(ds_["p_max"].data).shape
    pii = ds_["pulse_intensity_integral"]
    assert np.asarray(pii.data).shape == shape == (21, 21, 31) and pii.attrs["units"] == "J/cm^2" and pii.attrs["long_name"]
    assert np.array_equal(raw["pulse_intensity_integral"], np.asarray(pii.data)) and np.asarray(pii.data).max() > 0
    dt, n_t = sf.pulse_time_axis([1e-3] * 3, shape, 0, 0, 0.5)
    assert raw["p_trace"].shape == (2, n_t) and raw["t"].shape == (n_t,) and raw["t"][1] - raw["t"][0] == dt and raw["t"][0] == 0.0
    assert np.array_equal(raw["trace_voxels"], [(10 * 21 + 10) * 31 + 25, (13 * 21 + 10) * 31 + 20])
    # the traces are the waveforms behind the peak volumes of the same call
    for i, v in enumerate(raw["trace_voxels"]):
        assert abs(max(0.0, raw["p_trace"][i].max()) - raw["p_max"].ravel()[v]) <= 1e-6 * raw["p_max"].max()
    for key in ("p_max", "p_min", "intensity"):
        assert np.array_equal(np.asarray(ds_[key].data), np.asarray(plain_ds[key].data)), key


# ---- 13. thermal coupling -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_thermal_pulse_energy_source():
    arr = ol.Transducer.gen_matrix_array(nx=8, ny=8, pitch=2, kerf=0.2, units="mm", sensitivity=1e5)
    setup = ol.SimSetup(spacing=1.0, x_extent=(-8, 8), y_extent=(-8, 8), z_extent=(4, 28))
    # water with the absorption of the reference's example protocol (the stock water material has none: nothing would heat)
    water = ol.seg.seg_methods.UniformWater(materials={"water": Material("water", 1500.0, 1000.0, 0.0022, 4182.0, 0.598)})
    proto = ol.Protocol(pulse=ol.Pulse(frequency=F0, duration=2e-5), seg_method=water,
                        sequence=ol.Sequence(pulse_interval=0.1, pulse_count=9, pulse_train_interval=1.0, pulse_train_count=1),
                        focal_pattern=ol.focal_patterns.Wheel(center=True, num_spokes=2, spoke_radius=2.0, target_pressure=1e6),
                        sim_setup=setup, apod_method=ol.apod_methods.Uniform())
    sol, _, _ = proto.calc_solution(ol.Point(position=(0, 0, 20), units="mm"), arr, simulate=True, scale=True)
    params = setup.setup_sim_scene(water)
    base = np.asarray(run_thermal_simulation(params, sol)[0]["temperature_rise_max"].data)
    assert base.max() > 0
    E = np.asarray(sol.simulation_result["intensity"].data, dtype=np.float64) * min(2e-5, 0.1)
    same_ds, same_raw = run_thermal_simulation(params, sol, pulse_energy=E)
    assert same_raw["source"] == "pulse_energy"
    assert np.array_equal(np.asarray(same_ds["temperature_rise_max"].data), base)          # the same source, so the same run
    half = np.asarray(run_thermal_simulation(params, sol, pulse_energy=0.5 * E)[0]["temperature_rise_max"].data)
    # the scheme is linear in the source (atol: only fp32 denormals lose bits when halved)
    assert np.allclose(half, 0.5 * base, rtol=1e-6, atol=1e-30)


# ---- 14. the debug library -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_pii_and_trace_kernels_stay_inside_their_extents_in_the_debug_library():
    env = dict(os.environ, OLX_LIB_PATH=os.path.join(LIB, "libolx_dbg.so"))
    sel = "pii_matches_oracle_small or traces_match_oracle or window_longer or large_trace"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", sel, "-p", "no:cacheprovider"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=1800)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in tail and "failed" not in tail, tail
