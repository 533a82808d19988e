"""Full-wave model without a GPU: the host helpers of openlifu_amd/sim/fullwave.py, and the physics of the fp64 oracle
(tests/fullwave_oracle.py) against three known answers, so that the scheme itself is pinned on the CPU.

Known answers, each at two resolutions (8 and 12 points per wavelength at 500 kHz in water): the deviation must shrink on the finer
grid, and the coarse-grid deviation stays within its recorded value plus half again (DESIGN.md section 2 "full-wave model"; a
discretisation error has no rounding noise to allow for).  Measured with this oracle (coarse / fine):
  monopole A / r at 1.2 / 2.1 / 3.0 mm      7.51e-2 / 2.50e-2   (largest of the three radii)
  focal p_min of a 4 x 4 array vs the pulsed oracle   5.91e-2 / 1.37e-2
  decay through an absorbing slab vs exp(-alpha L)    3.96e-3 / 1.56e-3"""
import inspect
import logging

import numpy as np
import pytest

import openlifu_amd as ol
from openlifu_amd import _native as nat
from openlifu_amd.sim import fullwave as fw
from openlifu_amd.sim import run_fullwave_simulation, run_simulation
import fullwave_oracle as fo
import pulsed_oracle as po

F0, C0, RHO = 500e3, 1500.0, 1000.0
H_COARSE, H_FINE = 0.375e-3, 0.25e-3        # 8 and 12 points per wavelength
MONOPOLE_COARSE = 7.51e-2
FOCUS_COARSE = 5.91e-2
SLAB_COARSE = 3.96e-3


# ---- host helpers -------------------------------------------------------------------------------------------------------------------
def test_time_axis_cfl_is_a_request_that_never_destabilises():
    h, n = (0.5e-3,) * 3, (21, 21, 21)
    dt_max = 6.0 / (7.0 * 1500.0 * np.sqrt(3.0) / 0.5e-3)
    dt, n_steps, bound, ppw = fw.fullwave_time_axis(h, n, 1500.0, F0, 3, cfl=0.3)
    assert bound == pytest.approx(dt_max, rel=1e-14) and bound * 1500.0 / 0.5e-3 == pytest.approx(0.4949, abs=1e-4)
    assert dt == pytest.approx(0.3 * 0.5e-3 / 1500.0, rel=1e-14)
    # the reference's SimSetup.cfl default of 0.5 is above the bound: clamped to 0.9 dt_max
    dt5 = fw.fullwave_time_axis(h, n, 1500.0, F0, 3, cfl=0.5)[0]
    assert dt5 == pytest.approx(0.9 * dt_max, rel=1e-14) and dt5 < dt_max
    assert ppw == pytest.approx(1500.0 / (F0 * 0.5e-3))


def test_time_axis_refuses_a_dt_above_the_bound():
    h, n = (0.5e-3,) * 3, (21, 21, 21)
    bound = fw.stability_bound(h, 2800.0)
    c = np.full(n, 1500.0); c[5] = 2800.0
    assert fw.fullwave_time_axis(h, n, c, F0, 3, dt=bound)[0] == bound
    with pytest.raises(ValueError, match="stability bound"):
        fw.fullwave_time_axis(h, n, c, F0, 3, dt=bound * (1 + 1e-9))
    for bad in (dict(dt=-1.0), dict(t_end=np.inf), dict(cfl=0.0)):
        with pytest.raises(ValueError):
            fw.fullwave_time_axis(h, n, c, F0, 3, **bad)


def test_time_axis_anisotropic_spacing_and_t_end_rule():
    h, n = (0.4e-3, 0.5e-3, 0.3e-3), (37, 29, 43)
    c = np.full(n, 1500.0); c[:, :, 20:] = 2800.0; c[0, 0, 0] = 1400.0
    delays = np.array([0.0, 3e-6, 1e-6])
    dt, n_steps, bound, ppw = fw.fullwave_time_axis(h, n, c, F0, 5, delays, cfl=0.3)
    assert bound == pytest.approx(6.0 / (7.0 * 2800.0 * np.sqrt(sum(1.0 / np.square(h)))), rel=1e-14)
    assert dt == pytest.approx(min(0.3 * 0.3e-3 / 2800.0, 0.9 * bound), rel=1e-14)
    t_end = np.sqrt(sum((np.array(n) * h) ** 2)) / 1400.0 + 3e-6 + 5 / F0
    assert n_steps == int(np.ceil(t_end / dt))
    assert ppw == pytest.approx(1400.0 / (F0 * 0.5e-3))
    assert fw.fullwave_time_axis(h, n, c, F0, 5, delays, dt=2e-8, t_end=2e-6)[:2] == (2e-8, 100)


def test_points_per_wavelength_warning(caplog):
    with caplog.at_level(logging.WARNING):
        fw.fullwave_time_axis((0.25e-3,) * 3, (9, 9, 9), 1500.0, F0, 3)
    assert not caplog.records
    with caplog.at_level(logging.WARNING):
        ppw = fw.fullwave_time_axis((0.5e-3,) * 3, (9, 9, 9), 1500.0, F0, 3)[3]
    assert ppw == pytest.approx(6.0) and any("points per wavelength" in r.getMessage() for r in caplog.records)


def test_source_table_weights_and_amplitude():
    n, h, origin = (9, 8, 7), (0.4e-3, 0.5e-3, 0.3e-3), (-1e-3, 2e-3, 5e-3)
    pos = np.array([[-1e-3 + 2.3 * 0.4e-3, 2e-3 + 4.6 * 0.5e-3, 5e-3 + 1.25 * 0.3e-3],     # off the voxels: 8 entries
                    [-1e-3 + 3 * 0.4e-3, 2e-3 + 2 * 0.5e-3, 5e-3 + 6 * 0.3e-3],             # on a voxel (the last of z): 1 entry
                    [-1e-3 + 7.5 * 0.4e-3, 2e-3 + 0 * 0.5e-3, 5e-3 + 0 * 0.3e-3]])          # on an edge: 2 entries
    area, apod, delays = np.array([1e-6, 2e-6, 3e-6]), np.array([1.0, 0.5, 0.0]), np.array([1e-6, 2e-6, 3e-6])
    c = np.full(n, 1500.0); c[3, 2, 6] = 2000.0
    dt, p0, c_ref = 4e-8, 1e5, 1500.0
    ijk, amp, tau, el = fw.source_table(pos, area, apod, delays, origin, h, n, c, c_ref, F0, p0, dt)
    assert [int(np.sum(el == e)) for e in range(3)] == [8, 1, 2]
    assert ijk[el == 1].tolist() == [[3, 2, 6]] and np.all(amp[el == 2] == 0) and np.all(tau[el == 0] == 1e-6)
    for e in range(2):
        A = apod[e] * p0 * area[e] * F0 / c_ref
        cv = c[tuple(ijk[el == e].T)]
        w = amp[el == e] / (dt * cv ** 2 * 4 * np.pi * A / (2 * np.pi * F0 * np.prod(h)))
        assert w.sum() == pytest.approx(1.0, rel=1e-12) and np.all(w > 0)
    first = dict(zip(map(tuple, ijk[el == 0]), amp[el == 0]))
    assert first[(2, 4, 1)] / first[(3, 5, 2)] == pytest.approx((0.7 * 0.4 * 0.75) / (0.3 * 0.6 * 0.25), rel=1e-9)


def test_source_table_refuses_an_element_outside_the_grid():
    n, h = (9, 8, 7), (0.4e-3,) * 3
    pos = np.array([[1e-3, 1e-3, 1e-3], [1e-3, 1e-3, 6.2 * 0.4e-3], [1e-3, -0.1e-3, 1e-3]])
    one = np.ones(3)
    with pytest.raises(ValueError, match="element 1 "):
        fw.source_table(pos, one, one, one * 0, (0, 0, 0), h, n, 1500.0, 1500.0, F0, 1.0, 1e-8)
    with pytest.raises(ValueError, match="element 2 "):
        fw.source_table(pos[[0, 0, 2]], one, one, one * 0, (0, 0, 0), h, n, 1500.0, 1500.0, F0, 1.0, 1e-8)


def test_padding_replicates_edges_and_crop_inverts_it():
    rng = np.random.default_rng(3)
    vol = rng.normal(size=(5, 4, 6))
    pad = fw.pad_volume(vol, 3)
    assert pad.shape == (11, 10, 12)
    assert np.array_equal(fw.crop_volume(pad, 3), vol)
    assert np.all(pad[:3, 3:-3, 3:-3] == vol[0]) and np.all(pad[3:-3, 3:-3, -3:] == vol[:, :, -1:])
    assert pad[0, 0, 0] == vol[0, 0, 0] and pad[-1, -1, -1] == vol[-1, -1, -1]
    assert fw.pad_volume(vol, 0).shape == vol.shape and np.array_equal(fw.crop_volume(vol, 0), vol)


def test_layer_profile_is_one_inside_and_monotone():
    d = fw.layer_profile(41, 0.5e-3, 8, 2.0, 1500.0, 1e-7)
    assert np.all(d[8:-8] == 1.0) and np.all(d[:8] < 1.0) and np.all(d[-8:] < 1.0)
    assert np.all(np.diff(d[:9]) > 0) and np.all(np.diff(d[-9:]) < 0) and np.array_equal(d, d[::-1])
    assert d[0] == pytest.approx(np.exp(-2.0 * 1500.0 / 0.5e-3 * 1e-7)) and d[7] == pytest.approx(np.exp(-2.0 * 1500.0 / 0.5e-3 * 1e-7 / 8 ** 4))
    assert np.allclose(d, fo.decay(41, 0.5e-3, 8, 2.0, 1500.0, 1e-7), rtol=1e-15, atol=0)
    assert np.all(fw.layer_profile(7, 0.5e-3, 0, 2.0, 1500.0, 1e-7) == 1.0)


def test_signature_leads_with_the_reference_seam():
    ref = list(inspect.signature(run_simulation).parameters.values())[:14]
    new = list(inspect.signature(run_fullwave_simulation).parameters.values())
    assert [p.name for p in new[:14]] == [p.name for p in ref]
    assert [p.name for p in ref] == ["arr", "params", "delays", "apod", "freq", "cycles", "amplitude", "dt", "t_end", "cfl", "bli_tolerance",
                                     "upsampling_rate", "gpu", "ref_values_only"]
    for a, b in zip(new[:14], ref):
        if a.name != "cfl":
            assert a.default == b.default, a.name
    assert new[9].default == 0.3
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in new[14:])
    assert [p.name for p in new[14:]] == ["pml_size", "pml_alpha", "ramp_cycles", "pulse_intensity_integral", "record_points"]
    assert new[14].default == 16 and new[15].default == 2.0
    assert ol.sim.run_fullwave_simulation is run_fullwave_simulation and "run_fullwave_simulation" in ol.sim.__all__


def _small_scene():
    arr = ol.Transducer.gen_matrix_array(nx=2, ny=2, pitch=1.0, kerf=0.1, units="mm", sensitivity=1e5)
    setup = ol.SimSetup(spacing=0.5, x_extent=(-3, 3), y_extent=(-3, 3), z_extent=(0, 6))
    return arr, setup.setup_sim_scene(ol.seg_methods.UniformWater())


def test_refusals_come_before_any_device_call():
    arr, params = _small_scene()
    with pytest.raises(ValueError, match="shape"):
        run_fullwave_simulation(arr, params, delays=np.zeros(3), freq=F0, cycles=2)
    with pytest.raises(ValueError, match="pml_size"):
        run_fullwave_simulation(arr, params, freq=F0, cycles=2, pml_size=-1)
    with pytest.raises(ValueError, match="stability bound"):
        run_fullwave_simulation(arr, params, freq=F0, cycles=2, dt=1e-6)
    far = ol.Transducer.gen_matrix_array(nx=2, ny=2, pitch=20.0, kerf=0.1, units="mm", sensitivity=1e5)
    with pytest.raises(ValueError, match="element 0 "):
        run_fullwave_simulation(far, params, freq=F0, cycles=2)


def test_native_error_without_a_gpu():
    if nat.device_count() > 0:
        pytest.skip("GPU present")
    arr, params = _small_scene()
    with pytest.raises(nat.NativeError):
        run_fullwave_simulation(arr, params, freq=F0, cycles=2, pml_size=4)


# ---- physics of the oracle ------------------------------------------------------------------------------------------------------------
def monopole_deviation(h, pml=12, radii=(1.2e-3, 2.1e-3, 3.0e-3), A=1000.0):
    """One off-grid monopole at the centre of a water cube: steady amplitude on the +z line at three radii against A / r."""
    half = int(round(3.4e-3 / h))
    n = (2 * half + 1 + 2 * pml,) * 3
    src = np.array([(pml + half + 0.3) * h, (pml + half + 0.45) * h, (pml + half + 0.6) * h])
    dt = 0.3 * h / C0
    ijk, amp, tau = fo.monopole_entries(src[None], (0, 0, 0), h, [A], [0.0], C0, F0, dt, n)
    pts = np.array([(pml + half, pml + half, int(round((src[2] + r) / h))) for r in radii])
    rr = np.sqrt(((pts * h - src) ** 2).sum(axis=1))
    steps = int(np.ceil((rr.max() / C0 + 4 / F0) / dt))
    tr = fo.simulate(n, h, C0, RHO, 0.0, C0, pml, 2.0, dt, steps, ijk, amp, tau, F0, 14, 0.0, trace_ijk=pts)["trace"]
    t = (np.arange(steps) + 1) * dt
    dev = []
    for q, r in enumerate(rr):
        m = (t > r / C0 + 1.5 / F0) & (t < r / C0 + 3.5 / F0)
        dev.append(abs(np.abs(tr[m, q]).max() - A / r) / (A / r))
    return max(dev)


def test_oracle_monopole_reproduces_A_over_r():
    coarse, fine = monopole_deviation(H_COARSE), monopole_deviation(H_FINE)
    print(f"monopole deviation: coarse {coarse:.3e}, fine {fine:.3e}")
    assert fine < coarse
    assert coarse <= 1.5 * MONOPOLE_COARSE


def focus_deviation(h, pml=12):
    """Focal p_min of a 4 x 4 array (pitch 1.5 mm) focused 4.5 mm above its centre, against the pulsed oracle's Rayleigh sum."""
    half = int(round(3.6e-3 / h))
    nz = int(round(6.0e-3 / h))
    n = (2 * half + 1 + 2 * pml, 2 * half + 1 + 2 * pml, nz + 2 * pml)
    ctr = np.array([(pml + half) * h, (pml + half) * h, (pml + 1.5) * h])
    g = (np.arange(4) - 1.5) * 1.5e-3
    pos = np.array([[ctr[0] + x + 0.2 * h, ctr[1] + y + 0.35 * h, ctr[2]] for x in g for y in g])
    kf = int(round((ctr[2] + 4.5e-3) / h))
    focus = np.array([(pml + half) * h, (pml + half) * h, kf * h])
    d = np.sqrt(((pos - focus) ** 2).sum(axis=1))
    delays = (d.max() - d) / C0
    area, apod, p0, cycles = np.full(16, 1e-6), np.ones(16), 1e5, 4.0
    A = apod * area * p0 * F0 / C0
    dt = 0.3 * h / C0
    ijk, amp, tau = fo.monopole_entries(pos, (0, 0, 0), h, A, delays, C0, F0, dt, n)
    steps = int(np.ceil((d.max() / C0 + cycles / F0 + 1 / F0) / dt))
    out = fo.simulate(n, h, C0, RHO, 0.0, C0, pml, 2.0, dt, steps, ijk, amp, tau, F0, cycles, 0.0)
    got = out["p_min"][pml + half, pml + half, kf]
    dtp = 1.0 / (F0 * 400)          # the pulsed oracle on a fine time axis of its own; its delays are whole steps of it
    ref = po.pulsed_points(focus[None], pos, area, (np.floor(delays / dtp) + 0.5) * dtp, apod, F0, C0, p0, cycles, dtp, int(steps * dt / dtp), h / 2)[1][0]
    return abs(got - ref) / ref


def test_oracle_focal_pressure_matches_the_pulsed_oracle():
    coarse, fine = focus_deviation(H_COARSE), focus_deviation(H_FINE)
    print(f"focal p_min deviation: coarse {coarse:.3e}, fine {fine:.3e}")
    assert fine < coarse
    assert coarse <= 1.5 * FOCUS_COARSE


def slab_deviation(h, pml=10, alpha=80.0):
    """A sheet of in-phase monopoles sends a plane-like wave through a slab of water's c and rho that absorbs alpha [Np/m].  On the axis
    behind the slab, until the edge wave of the finite sheet arrives (0.7 periods after the plane wave), the trace is the trace of the
    same run without absorption times exp(-alpha L): the least-squares ratio of the two against that."""
    half = int(round(4.5e-3 / h))
    gap, thick = int(round(0.75e-3 / h)), int(round(2.25e-3 / h))
    n = (2 * half + 1 + 2 * pml, 2 * half + 1 + 2 * pml, 2 * gap + thick + 4 + 2 * pml)
    ks = pml + 1
    k0, k1 = ks + gap, ks + gap + thick
    kp = k1 + gap
    L = thick * h
    a = np.zeros(n); a[:, :, k0:k1] = alpha
    ii, jj = np.meshgrid(np.arange(pml, pml + 2 * half + 1), np.arange(pml, pml + 2 * half + 1), indexing="ij")
    ijk = np.stack([ii.ravel(), jj.ravel(), np.full(ii.size, ks)], axis=1)
    dt = 0.3 * h / C0
    amp, tau = np.full(ijk.shape[0], 1.0), np.zeros(ijk.shape[0])
    pt = np.array([[pml + half, pml + half, kp]])
    dist = (kp - ks) * h
    edge = np.sqrt(dist ** 2 + (half * h) ** 2)
    steps = int(np.floor(min(edge / C0, dist / C0 + 0.65 / F0) / dt))
    with_a, without = (fo.simulate(n, h, C0, RHO, med, C0, pml, 2.0, dt, steps, ijk, amp, tau, F0, 3.0, 0.0, trace_ijk=pt)["trace"][:, 0] for med in (a, 0.0))
    ratio = float(with_a @ without / (without @ without))
    return abs(ratio - np.exp(-alpha * L)) / np.exp(-alpha * L)


def test_oracle_absorbing_slab_decays_as_exp_minus_alpha_x():
    coarse, fine = slab_deviation(H_COARSE), slab_deviation(H_FINE)
    print(f"slab decay deviation: coarse {coarse:.3e}, fine {fine:.3e}")
    assert fine < coarse
    assert coarse <= 1.5 * SLAB_COARSE
