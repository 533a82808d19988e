"""Pulsed (tone-burst) field model through a heterogeneous medium on the MI355X: kernel 2ph (field_pulse_med_k, olx_field_pulse_medium) through
the C-ABI against the fp64 oracle (tests/pulsed_medium_oracle.py), its limits (trivial medium = kernel 2p, long burst = kernel 2h, late
arrivals), PII and traces, run_simulation / Protocol.calc_solution with the opt-in medium model, and the debug library.
Gates: p_max / p_min <= 1e-5 of the volume maximum, voxels whose t_e / dt or (t_e + T) / dt lies within 1e-7 of an
integer excluded (fewer than 0.1 %), intensity rtol 1e-5 with the voxel's own impedance, PII <= 4e-5 of its maximum, traces <= 1e-5 of the
largest sample.  The cases are tests/pulsed_medium_cases.py's."""
import os
import subprocess
import sys

import numpy as np
import pytest

import openlifu_amd as ol
from openlifu_amd import _native as nat
from openlifu_amd.bf.delay_methods import StraightRay
from openlifu_amd.seg.material import Material
from openlifu_amd.seg.seg_methods.threshold import SkullThreshold
from openlifu_amd.sim import field as sf
from openlifu_amd.util import dataset as ds
import pulsed_medium_oracle as pmo
import pulsed_medium_cases as pc
from pulsed_medium_cases import C, F0, P0, RHO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "openlifu-python_amd", "lib")
TOL, MARGIN, MAX_EXCLUDED, TOL_PII = 1e-5, 1e-7, 1e-3, 4e-5


@pytest.fixture(scope="module")
def ctx():
    c = nat.Context(0)
    yield c
    c.close()


def launch(ctx, k, ss="case", att="case", rho=None, delays=None, flags=0, medium=True, trace=None, also_2p=False):
    """One pulsed launch of case k through (ss, att, rho) ("case" = the case's volume, None = absent) -> (outputs, variant string).
    ``also_2p``: kernel 2p's launch of the same plan first, returned as a third value."""
    ss = k.ss if isinstance(ss, str) else ss
    att = k.att if isinstance(att, str) else att
    ctx.set_elements(k.pos_m, np.tile([0.0, 0.0, 1.0], (len(k.pos_m), 1)), k.area)
    ctx.set_steering(k.delays if delays is None else delays, k.apod)
    ctx.field_absorption(0.0)
    ctx.field_pulse(k.cycles, k.dt, k.n_t)
    want = ("pmag", "intensity", "pmax") + (("pii",) if flags & nat.OUT_PII else ())
    try:
        ctx.field_plan(k.origin, k.spacing, k.n, F0, C, RHO, P0, flags=nat.OUT_PMAG | nat.OUT_INTENSITY | nat.OUT_PMAX | flags)
        plain = None
        if also_2p:
            assert ctx.field_variant().startswith("field_pulse_k ")
            ctx.field_launch()
            plain = ctx.field_fetch_all(want=want)
        if medium:
            ctx.field_pulse_medium(ss, att, rho)
        variant = ctx.field_variant()
        ctx.field_launch()
        out = ctx.field_fetch_all(want=want)
        if trace is not None:
            out["trace"] = ctx.field_pulse_trace(trace)
        ctx.sync()
    finally:
        ctx.field_pulse(0.0, 0.0, 0)
    return (out, variant, plain) if also_2p else (out, variant)


def check_gate(out, refs, z=RHO * C, label=""):
    """Per focus: p_max / p_min over the included voxels within TOL of the oracle's volume maximum, the intensity with impedance z."""
    for f, (omax, omin, margin) in enumerate(refs):
        ok = margin >= MARGIN
        assert (~ok).mean() < MAX_EXCLUDED, f"{(~ok).mean():.2e} of the voxels excluded"
        for gpu, o, name in ((out["pmax"][f], omax, "p_max"), (out["pmag"][f], omin, "p_min")):
            e = np.abs(gpu.astype(np.float64) - o)[ok].max() / o.max()
            print(f"{label} focus {f} {name}: error {e:.3e} of the volume maximum")
            assert e <= TOL, f"{label} focus {f} {name}: error {e:.3e} of the volume maximum"
        it = 1e-4 * out["pmag"][f].astype(np.float64) ** 2 / (2 * z)
        assert np.allclose(out["intensity"][f], it, rtol=1e-5, atol=1e-7 * it.max()), f"{label} focus {f} intensity"


# ---- 1. the kernel against the oracle, full volumes ----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["slab16", "slab64_2foci", "inside16", "below16", "n1", "n65", "n300", "two_pass"])
def test_pulsed_medium_kernel_matches_oracle(ctx, name):
    k = pc.case(name)
    out, variant = launch(ctx, k)
    assert variant.startswith("field_pulse_med_k (pulsed through a medium: ") and f"{k.n_t} samples" in variant
    assert f"R = {4 if len(k.pos_m) <= 256 else 16}" in variant, variant
    refs = [k.oracle(f) for f in range(len(k.foci_m))]
    check_gate(out, refs, z=k.ss.astype(np.float64) * RHO, label=name)      # (no density volume: rho is the plan's)
    assert refs[0][0].max() > 0
    if name == "two_pass":
        assert k.cycles / (F0 * k.dt) > 64 * 21
    if name in ("inside16", "below16"):      # both branches of the plane bounds are on the rays
        assert (k.pos_m[:, 2] > k.origin[2]).all() and (k.pos_m[:, 2] < k.origin[2] + (k.n[2] - 1) * 1e-3).all()
    if name == "slab64_2foci":
        assert not np.array_equal(out["pmag"][0], out["pmag"][1])
        # the medium's parts one at a time, and the intensity with a density volume
        for label, kw, sel in (("absorbing-only", dict(ss=None), dict(ss=False)), ("lossless", dict(att=None), dict(att=False))):
            o2, _ = launch(ctx, k, **kw)
            z = (k.ss.astype(np.float64) if kw.get("ss", "case") is not None else C) * RHO
            check_gate(o2, [k.oracle(f, **sel) for f in range(2)], z=z, label=f"{name} {label}")
        o3, _ = launch(ctx, k, rho=k.rho)
        check_gate(o3, refs, z=k.ss.astype(np.float64) * k.rho.astype(np.float64), label=f"{name} density")
        assert np.array_equal(o3["pmag"], out["pmag"]) and np.array_equal(o3["pmax"], out["pmax"])


@pytest.mark.gpu
def test_pulsed_medium_with_straightray_delays(ctx):
    """slab16 again with the delays of kernel 1m (olx_bf_solve_medium) through the same sound-speed volume."""
    k = pc.case("slab16")
    ctx.set_elements(k.pos_m, np.tile([0.0, 0.0, 1.0], (len(k.pos_m), 1)), k.area)
    ctx.bf_set_medium(k.ss, k.origin, k.spacing, k.n, C)
    delays, _ = ctx.bf_solve_medium(k.foci_m, C)
    assert not np.allclose(delays, k.delays, rtol=0, atol=1e-8)
    out, _ = launch(ctx, k, delays=delays)
    check_gate(out, [k.oracle(0, delays=delays)], z=k.ss.astype(np.float64) * RHO, label="slab16 StraightRay")
    direct, _ = launch(ctx, k)
    fi = tuple(int(v) for v in np.rint((k.foci_m[0] - np.asarray(k.origin)) / 1e-3))
    print(f"slab16 p_min at the focus: StraightRay {out['pmag'][0][fi]:.4e} Pa, Direct {direct['pmag'][0][fi]:.4e} Pa")


# ---- 2. PII and traces -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def traced(ctx):
    """slab16 with a density volume, OLX_OUT_PII and the traces of the focus voxel plus 8 seeded points, launched once."""
    k = pc.case("slab16")
    fi = np.rint((k.foci_m[0] - np.asarray(k.origin)) / 1e-3).astype(np.int64)
    rng = np.random.default_rng(77)
    idx = np.vstack([fi[None, :], np.stack([rng.integers(0, k.n[a], size=8) for a in range(3)], axis=1)])
    lin = np.ravel_multi_index(tuple(idx.T), k.n)
    out, _ = launch(ctx, k, rho=k.rho, flags=nat.OUT_PII, trace=lin)
    return k, idx, lin, out


@pytest.mark.gpu
def test_pulsed_medium_pii_and_traces(traced):
    k, idx, lin, out = traced
    A, E = k.sums()
    p, margin = pmo.pulsed_medium_waveforms(k.origin, k.spacing, k.n, k.pos_m, k.area, k.delays[0], k.apod[0], F0, C, P0, k.cycles, k.dt, k.n_t, A, E)
    z = pmo.impedance(k.n, RHO, C, k.ss, k.rho)
    pii = pmo.pulsed_medium_pii(p, k.dt, z).reshape(k.n)
    ok = (margin >= MARGIN).reshape(k.n)
    assert (~ok).mean() < MAX_EXCLUDED
    e = np.abs(out["pii"][0].astype(np.float64) - pii)[ok].max() / pii.max()
    print(f"slab16 PII: error {e:.3e} of its maximum")
    assert e <= TOL_PII, e
    tr = out["trace"][0]
    assert tr.shape == (9, k.n_t)
    et = np.abs(tr.astype(np.float64) - p[lin]).max() / np.abs(p[lin]).max()
    print(f"slab16 traces: error {et:.3e} of the largest sample")
    assert margin[lin].min() >= MARGIN and et <= TOL
    # exact zeros outside [first arrival, last burst end)
    u, _ = pmo.arrival_steps(np.asarray(k.origin)[None, :] + idx * 1e-3, k.pos_m, k.delays[0], k.dt, C, 0.5e-3, E[lin])
    for q in range(9):
        k0, k1 = int(np.ceil(u[q]).min()), int(np.ceil(u[q] + k.cycles / (F0 * k.dt)).max())
        assert np.all(tr[q, :k0] == 0.0) and np.all(tr[q, min(k1, k.n_t):] == 0.0)
        assert tr[q, k0] != 0.0


@pytest.mark.gpu
def test_trace_peaks_are_the_volumes_bit_for_bit(traced):
    """As DESIGN.md section 5.7 records for kernel 2p: the product library's trace and volume instantiations evaluate the same sums in
    the same order.  (Not part of the debug-library run: its index checks change the order in which the lanes' fp32 terms meet in LDS.)"""
    k, idx, lin, out = traced
    tr = out["trace"][0]
    assert np.array_equal(np.maximum(tr.max(axis=1), 0.0), out["pmax"][0].ravel()[lin])
    assert np.array_equal(np.maximum(-tr.min(axis=1), 0.0), out["pmag"][0].ravel()[lin])


# ---- 3. limits -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_trivial_medium_is_kernel_2p(ctx):
    """Volumes equal to the reference values everywhere (no non-trivial plane): kernel 2ph's result lies within twice the fp32 rounding of
    an amplitude sum of kernel 2p's launch of the same plan."""
    k = pc.case("slab16")
    out, variant, plain = launch(ctx, k, ss=np.full(k.n, C, dtype=np.float32), att=np.zeros(k.n, dtype=np.float32), rho=np.full(k.n, RHO, dtype=np.float32),
                                 also_2p=True)
    assert variant.startswith("field_pulse_med_k (pulsed through a medium: ") and " 0 planes" in variant, variant
    for key in ("pmax", "pmag"):
        e = np.abs(out[key].astype(np.float64) - plain[key]).max() / plain[key].max()
        print(f"trivial medium vs kernel 2p, {key}: {e:.3e} of the maximum")
        assert e <= 2e-6, (key, e)
    assert np.allclose(out["intensity"], plain["intensity"], rtol=1e-5, atol=1e-7 * plain["intensity"].max())


@pytest.mark.gpu
def test_pulsed_medium_long_burst_approaches_kernel_2h(ctx):
    """The form of test_pulsed_long_burst_approaches_cw, through the slab: kernel 2h (sampled) fed the truncated delays is the steady state."""
    K = 16
    k = pc.case("cw_limit")
    out, _ = launch(ctx, k)
    ctx.set_steering(sf.truncate_delays(k.delays, k.dt), k.apod)
    ctx.field_plan(k.origin, k.spacing, k.n, F0, C, RHO, P0, flags=nat.OUT_PMAG | nat.FIELD_FP16_CORRECTION)
    ctx.field_set_medium(k.ss, k.att, None, model="sampled")
    assert "hetero" in ctx.field_variant()
    ctx.field_launch()
    cw = ctx.field_fetch_all(want=("pmag",))["pmag"][0]
    ctx.sync()
    idx = pmo.voxel_indices(k.n)
    u, _ = pmo.arrival_steps(np.asarray(k.origin)[None, :] + idx * 1e-3, k.pos_m, k.delays[0], k.dt, C, 0.5e-3, k.sums()[1])
    lo, hi = u.max(1), np.minimum((u + k.cycles * K).min(1), k.n_t - 1)
    full = (hi - lo >= K + 1).reshape(cw.shape)          # the full-overlap interval spans at least one period of samples
    assert full.mean() > 0.5
    tol = 2e-5 * cw.max()                                # (the two kernels' gates added)
    pm = out["pmax"][0]
    assert np.all(pm[full] >= np.cos(np.pi / K) * cw[full] - tol)
    beam = full & (cw >= 0.5 * cw.max())
    assert beam.sum() > 10
    assert np.all(pm[beam] <= cw[beam] + tol)


@pytest.mark.gpu
def test_pulsed_medium_late_arrivals_give_exact_zero(ctx):
    k = pc.case("late16")
    out, _ = launch(ctx, k, rho=k.rho, flags=nat.OUT_PII)
    idx = pmo.voxel_indices(k.n)
    u, _ = pmo.arrival_steps(np.asarray(k.origin)[None, :] + idx * 1e-3, k.pos_m, k.delays[0], k.dt, C, 0.5e-3, k.sums()[1])
    late = (np.ceil(u.min(1) - 1e-7) >= k.n_t).reshape(k.n)
    assert 0.05 < late.mean() < 0.95
    for key in ("pmax", "pmag", "intensity", "pii"):
        assert np.all(out[key][0][late] == 0.0), key
    assert np.all(out["pmag"][0][~late] >= 0.0) and out["pmag"][0][~late].max() > 0
    check_gate(out, [k.oracle(0)], z=k.ss.astype(np.float64) * k.rho.astype(np.float64), label="late16")


@pytest.mark.gpu
def test_pulsed_medium_refusals(ctx):
    k = pc.case("n1")
    ctx.set_elements(k.pos_m, np.tile([0.0, 0.0, 1.0], (1, 1)), k.area)
    ctx.set_steering(k.delays, k.apod)
    ctx.field_pulse(0.0, 0.0, 0)
    ctx.field_plan(k.origin, k.spacing, k.n, F0, C, RHO, P0, flags=nat.OUT_PMAG)
    with pytest.raises(nat.NativeError, match="needs a pulsed plan"):
        ctx.field_pulse_medium(k.ss, k.att, None)
    try:
        ctx.field_pulse(k.cycles, k.dt, k.n_t)
        ctx.field_absorption(2.0)
        ctx.field_plan(k.origin, k.spacing, k.n, F0, C, RHO, P0, flags=nat.OUT_PMAG)
        with pytest.raises(ValueError, match="uniform absorption"):
            ctx.field_pulse_medium(k.ss, k.att, None)
        ctx.field_absorption(0.0)
        ctx.field_plan(k.origin, k.spacing, k.n, F0, C, RHO, P0, flags=nat.OUT_PMAG)
        with pytest.raises(ValueError, match="no heterogeneous-medium kernel"):
            ctx.field_set_medium(k.ss, k.att, None)              # the CW call keeps refusing a pulsed plan
        ctx.field_pulse_medium(k.ss, k.att, None)
        assert ctx.field_variant().startswith("field_pulse_med_k")
        ctx.field_plan(k.origin, k.spacing, k.n, F0, C, RHO, P0, flags=nat.OUT_PMAG)
        assert ctx.field_variant().startswith("field_pulse_k ")    # the next plan clears the medium
        # more elements than the cache holds
        n = 1025
        pos = np.zeros((n, 3)); pos[:, 0] = (np.arange(n) - n / 2) * 1e-4
        ctx.set_elements(pos, np.tile([0.0, 0.0, 1.0], (n, 1)), np.full(n, 1e-8))
        ctx.set_steering(np.zeros((1, n)), np.ones((1, n)))
        ctx.field_plan(k.origin, k.spacing, k.n, F0, C, RHO, P0, flags=nat.OUT_PMAG)
        with pytest.raises(ValueError, match="1024"):
            ctx.field_pulse_medium(k.ss, k.att, None)
    finally:
        ctx.field_pulse(0.0, 0.0, 0)
        ctx.field_absorption(0.0)


# ---- 4. Python end to end ----------------------------------------------------------------------------------------------------------------
def _scene():
    setup = ol.SimSetup(spacing=1.0, x_extent=(-6, 6), y_extent=(-5, 5), z_extent=(4, 24))
    params = setup.setup_sim_scene(ol.seg.seg_methods.UniformWater())
    shape = params["sound_speed"].shape
    ss, att, rho = pc.wavy_slab(shape, 5, 9)
    for key, vol in (("sound_speed", ss), ("attenuation", att), ("density", rho)):
        old = params[key]
        params[key] = ds.make_dataarray(vol, coords={d: old.coords[d] for d in old.dims}, dims=old.dims, name=key, attrs=dict(old.attrs))
    return setup, params


@pytest.mark.gpu
def test_run_simulation_pulsed_through_a_medium_schema():
    arr = ol.Transducer.gen_matrix_array(nx=4, ny=4, pitch=3, kerf=0.3, units="mm", sensitivity=1e5)
    _, params = _scene()
    pts = np.array([[0.0, 0.0, 20.0], [2.0, -1.0, 12.0]])
    ds_, raw = sf.run_simulation(arr, params, freq=F0, cycles=4, amplitude=1, field_model="pulsed", medium_model="straight_ray",
                                 pulse_intensity_integral=True, record_points=pts)
    assert np.array_equal(raw["p_max"], np.asarray(ds_["p_max"].data)) and np.array_equal(raw["p_min"], -np.asarray(ds_["p_min"].data))
    assert np.array_equal(raw["pulse_intensity_integral"], np.asarray(ds_["pulse_intensity_integral"].data))
    assert raw["p_trace"].shape == (2, len(raw["t"])) and raw["p_max"].max() > 0 and raw["pulse_intensity_integral"].max() > 0
    # through the slab, not through water: the homogeneous reference run differs
    _, ref = sf.run_simulation(arr, params, freq=F0, cycles=4, amplitude=1, field_model="pulsed", ref_values_only=True)
    assert not np.allclose(ref["p_max"], raw["p_max"], rtol=1e-2, atol=1e-3 * raw["p_max"].max())
    # a homogeneous params with the opt-in runs kernel 2p (the rule of the steering map)
    water = ol.SimSetup(spacing=1.0, x_extent=(-6, 6), y_extent=(-5, 5), z_extent=(4, 24)).setup_sim_scene(ol.seg.seg_methods.UniformWater())
    a = sf.run_simulation(arr, water, freq=F0, cycles=4, field_model="pulsed", medium_model="straight_ray")[1]
    assert ol.get_engine().ctx.field_variant().startswith("field_pulse_k ")
    b = sf.run_simulation(arr, water, freq=F0, cycles=4, field_model="pulsed")[1]
    assert np.array_equal(a["p_max"], b["p_max"]) and np.array_equal(a["p_min"], b["p_min"])


@pytest.mark.gpu
def test_calc_solution_pulsed_through_a_medium_end_to_end():
    mats = {"water": Material("water", 1500.0, 1000.0, 0.0, 4182.0, 0.598), "skull": Material("skull", 2800.0, 1900.0, 4.0, 1300.0, 0.4),
            "tissue": Material("tissue", 1540.0, 1050.0, 0.3, 3600.0, 0.528)}
    setup = ol.SimSetup(spacing=1.0, x_extent=(-6, 6), y_extent=(-5, 5), z_extent=(4, 24),
                        options={"field_model": "pulsed", "pulsed_medium_model": "straight_ray"})
    proto = ol.Protocol(pulse=ol.Pulse(frequency=F0, duration=2e-5), sequence=ol.Sequence(pulse_interval=0.1, pulse_count=4),
                        focal_pattern=ol.focal_patterns.Wheel(center=True, num_spokes=1, spoke_radius=2.0, target_pressure=1e6), sim_setup=setup,
                        seg_method=SkullThreshold(materials=mats), apod_method=ol.apod_methods.Uniform())
    proto.delay_method = StraightRay()
    coords = setup.get_coords()
    xs, ys, zs = (np.asarray(c.data) * 1e-3 for c in coords.values())
    zr = zs[None, None, :] - 0.2 * xs[:, None, None]          # a flat slab tilted about y
    img = np.ascontiguousarray(np.broadcast_to(np.where((zr >= 8e-3) & (zr < 12e-3), 1000.0, 0.0), (len(xs), len(ys), len(zs))).astype(np.float32))
    vol = ds.make_dataarray(img, coords=coords, dims=list(coords.keys() if not hasattr(coords, "dims") else coords.dims), name="ct")
    arr = ol.Transducer.gen_matrix_array(nx=8, ny=8, pitch=2, kerf=0.2, units="mm", sensitivity=1e5)
    target = ol.Point(position=(0, 0, 18), units="mm")
    sol, agg, analysis = proto.calc_solution(target, arr, volume=vol, simulate=True, scale=True)
    assert ol.get_engine().ctx.field_variant().startswith("field_pulse_med_k")
    res = sol.simulation_result
    pmax, pmin = (np.array(res[key].data) for key in ("p_max", "p_min"))
    assert pmax.shape[0] == 2 and not np.array_equal(pmax, pmin)
    assert np.allclose(analysis.mainlobe_pnp_MPa, 1.0, rtol=1e-5)
    assert np.array_equal(np.asarray(agg["p_max"].data), pmax.max(axis=0))
    assert np.array_equal(np.asarray(agg["p_min"].data), pmin.max(axis=0))
    # without the opt-in the same protocol is refused in the words of the plain call
    del setup.options["pulsed_medium_model"]
    with pytest.raises(NotImplementedError, match="heterogeneous media are not implemented"):
        proto.calc_solution(target, arr, volume=vol, simulate=True, scale=True)


# ---- 5. the debug library ------------------------------------------------------------------------------------------------------------------
def test_pulsemed_bounds_tag_only_in_the_debug_library():
    prod = open(os.path.join(LIB, "libolx.so"), "rb").read()
    dbg = open(os.path.join(LIB, "libolx_dbg.so"), "rb").read()
    assert b"olx_dbg_bounds_pulsemed" in dbg and b"olx_dbg_bounds_pulsemed" not in prod


@pytest.mark.gpu
def test_pulsed_medium_kernels_stay_inside_their_extents_in_the_debug_library():
    env = dict(os.environ, OLX_LIB_PATH=os.path.join(LIB, "libolx_dbg.so"))
    sel = "matches_oracle or late_arrivals or pii_and_traces"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", sel, "-p", "no:cacheprovider"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in tail and "failed" not in tail, tail
