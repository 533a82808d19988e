"""MediumCompensated apodization on the MI355X: kernel 1a through the C-ABI against the fp64 oracle (tests/medium_apod_oracle.py), the base
apodization bit for bit without attenuation, the one-walk pairing with StraightRay against the two seams, the sampled field model reading the
resident table, the state the new exports leave alone, calc_solution end to end on the skull protocol, and the debug library (DESIGN.md
section 2 "MediumCompensated", section 5.10).  Phantom, arrays, foci and transform: tests/test_gpu_medium_delays.py's."""
import os
import subprocess
import sys

import numpy as np
import pytest

import openlifu_amd as ol
from openlifu_amd import _native as nat
from openlifu_amd.bf.apod_methods import MaxAngle, MediumCompensated
from openlifu_amd.bf.delay_methods import Direct, StraightRay
from openlifu_amd.engine import grid_from_coords
import medium_apod_oracle as ao
import medium_delay_oracle as mo
from test_gpu_medium_delays import C, F0, LIB, P0, RHO, ROOT, _array, _elements, _grid, _skull, _skull_protocol, _volume

N, H = (25, 21, 30), 1e-3
BASES = {"uniform": (nat.APOD_UNIFORM, 1.0), "maxangle50": (nat.APOD_MAXANGLE, 50.0)}


def _case():
    origin, spacing, (xs, ys, zs) = _grid(N, H, 4e-3)
    foci = np.array([[xs[12], ys[10], zs[22]], [xs[3], ys[17], zs[11]],         # grid voxels (one inside the skull)
                     [1.3e-3, -2.7e-3, 25.35e-3], [0.2e-3, 0.4e-3, 9.5e-3],     # off the voxels (one between skull planes)
                     [19e-3, -15e-3, 27.5e-3], [-30e-3, 4e-3, 20e-3]])          # outside the lateral extent
    M = np.eye(4); M[:3, 3] = [0.4e-3, -0.3e-3, -0.5e-3]
    return origin, spacing, (xs, ys, zs), foci, M


@pytest.mark.gpu
@pytest.mark.parametrize("inside", [False, True])
def test_apodization_matches_oracle(ctx, inside):
    origin, spacing, (xs, ys, zs), foci, M = _case()
    cvol, avol = _skull(xs, ys, zs)
    pos_m, area = _elements(ctx, inside=inside)
    ctx.bf_set_attenuation(avol, origin, spacing, N, F0)
    for mat in (None, M):
        _, h_plain, _ = ao.arrival(pos_m, foci, avol, origin, spacing, F0, M=mat)
        _, h_spread, _ = ao.arrival(pos_m, foci, avol, origin, spacing, F0, area=area, M=mat)
        for base, (kind, p0) in BASES.items():
            d0, b = ctx.bf_solve(foci, C, matrix=mat, apod_kind=kind, p0=p0)
            assert (b > 0).sum() > len(foci)
            for mode in ("equalize", "matched"):
                for spreading, h in ((False, h_plain), (True, h_spread)):
                    d, a = ctx.bf_solve_compensated(foci, C, matrix=mat, apod_kind=kind, p0=p0, mode=mode, spreading=spreading)
                    ref = ao.compensate(b, h, mode)
                    err, moved = np.abs(a - ref).max(), np.abs(a - b).max()
                    print(f"kernel 1a vs oracle (inside={inside}, transform={mat is not None}, {base}, {mode}, spreading={spreading}): "
                          f"{err:.2e}, max |apod - b| {moved:.3f}")
                    assert err <= 1e-12, err
                    assert np.array_equal(a == 0, b == 0)
                    assert moved > 1e-3                                   # the medium matters here
                    assert (a <= b).all() and (a >= 0).all()
                    assert np.array_equal(d, d0)                          # kernel 1's delays


@pytest.mark.gpu
def test_no_attenuation_is_the_base_method_bit_for_bit(ctx):
    origin, spacing, (xs, ys, zs), foci, M = _case()
    cvol, _ = _skull(xs, ys, zs)
    _elements(ctx)
    for mat in (None, M):
        d0, b = ctx.bf_solve(foci, C, matrix=mat, apod_kind=nat.APOD_PIECEWISE, p0=60.0, p1=30.0)
        ctx.bf_set_medium(cvol, origin, spacing, N, C)
        d1, b1 = ctx.bf_solve_medium(foci, C, matrix=mat, apod_kind=nat.APOD_PIECEWISE, p0=60.0, p1=30.0)
        assert np.array_equal(b1, b) and not np.array_equal(d1, d0)
        for vol in (None, np.zeros(N, dtype=np.float32)):
            ctx.bf_set_attenuation(vol, origin, spacing, N, F0)
            for mode in ("equalize", "matched"):
                d, a = ctx.bf_solve_compensated(foci, C, matrix=mat, apod_kind=nat.APOD_PIECEWISE, p0=60.0, p1=30.0, mode=mode)
                assert np.array_equal(a, b) and np.array_equal(d, d0)
                d, a = ctx.bf_solve_compensated(foci, C, matrix=mat, apod_kind=nat.APOD_PIECEWISE, p0=60.0, p1=30.0, mode=mode,
                                                use_delay_medium=True)
                assert np.array_equal(a, b) and np.array_equal(d, d1)


@pytest.mark.gpu
@pytest.mark.parametrize("inside", [False, True])
def test_one_walk_equals_the_two_kernels(ctx, inside):
    """Delays and apodization of the one-walk launch (planes held by either volume) against olx_bf_solve_medium's delays and the
    attenuation-only launch's apodization, bit for bit; the lossy third layer's planes are held by both volumes, the skull's differ."""
    origin, spacing, (xs, ys, zs), foci, M = _case()
    cvol, avol = _skull(xs, ys, zs)
    avol[:, :, 26] = 0.4                     # a plane only the attenuation holds
    cvol[:, :, 2] = 1510.0                   # ... and one only the sound speed holds
    _elements(ctx, inside=inside)
    ctx.bf_set_medium(cvol, origin, spacing, N, C)
    ctx.bf_set_attenuation(avol, origin, spacing, N, F0)
    for mat in (None, M):
        for mode, spreading in (("equalize", True), ("matched", False)):
            d1, _ = ctx.bf_solve_medium(foci, C, matrix=mat, apod_kind=nat.APOD_MAXANGLE, p0=50.0)
            _, a1 = ctx.bf_solve_compensated(foci, C, matrix=mat, apod_kind=nat.APOD_MAXANGLE, p0=50.0, mode=mode, spreading=spreading)
            d, a = ctx.bf_solve_compensated(foci, C, matrix=mat, apod_kind=nat.APOD_MAXANGLE, p0=50.0, mode=mode, spreading=spreading,
                                            use_delay_medium=True)
            assert np.array_equal(d, d1) and np.array_equal(a, a1)


@pytest.mark.gpu
def test_fused_protocol_equals_the_two_seams():
    """Protocol.beamform_foci with StraightRay + MediumCompensated (kernel 1 + one walk) against StraightRay.calc_delays and
    MediumCompensated.calc_apodization called separately, bit for bit; Direct + MediumCompensated likewise."""
    proto, setup = _skull_protocol(ol.focal_patterns.Wheel(center=True, num_spokes=3, spoke_radius=2.0, target_pressure=1e6),
                                   MediumCompensated(base=MaxAngle(max_angle=45.0), mode="matched", spreading=True))
    params = setup.setup_sim_scene(proto.seg_method, volume=_volume(setup))
    arr = _array()
    foci = proto.focal_pattern.get_targets(ol.Point(position=(0, 0, 20), units="mm"))
    own = MediumCompensated(base=MaxAngle(max_angle=45.0), mode="matched", spreading=True, frequency=proto.pulse.frequency)
    a_seam = own.calc_apodization(arr, foci, params)
    assert a_seam.shape == (4, 64) and np.array_equal(own.calc_apodization(arr, foci[1], params), a_seam[1])
    assert np.abs(a_seam - MaxAngle(max_angle=45.0).calc_apodization(arr, foci)).max() > 1e-3
    for dm in (StraightRay(), Direct()):
        proto.delay_method = dm
        d, a, resident = proto.beamform_foci(arr, foci, params)
        assert resident and np.array_equal(d, dm.calc_delays(arr, foci, params)) and np.array_equal(a, a_seam)
        d1, a1 = proto.beamform(arr, foci[2], params)
        assert np.array_equal(d1, d[2]) and np.array_equal(a1, a[2])
    assert np.array_equal(own.calc_apodization(arr, foci), MaxAngle(max_angle=45.0).calc_apodization(arr, foci))      # params=None: the base


@pytest.mark.gpu
@pytest.mark.parametrize("mode,spreading", [("equalize", True), ("matched", False)])
def test_the_sampled_field_uses_the_resident_table(ctx, mode, spreading):
    """Sampled field model (kernel 2h) launched on the resident table of the one-walk solve, at voxel foci behind the skull phantom:
    |p(focus)| = sum_e apod_e w_e exp(-A_e) / d_e of the fp64 oracle (w = p0 S / lambda), within the bound of
    test_gpu_medium_delays.py::test_exact_focusing_of_the_sampled_model_and_direct_falls_short for its coherent sum (1e-5)."""
    origin, spacing, (xs, ys, zs), _, _ = _case()
    cvol, avol = _skull(xs, ys, zs, third=False)
    pos_m, area = _elements(ctx)
    vox = [(12, 10, 22), (7, 14, 25), (15, 6, 19)]
    foci = np.array([[xs[i], ys[j], zs[k]] for i, j, k in vox])
    ctx.bf_set_medium(cvol, origin, spacing, N, C)
    ctx.bf_set_attenuation(avol, origin, spacing, N, F0)
    d, a = ctx.bf_solve_compensated(foci, C, apod_kind=nat.APOD_MAXANGLE, p0=50.0, mode=mode, spreading=spreading, use_delay_medium=True)
    ctx.field_plan(origin, spacing, N, F0, C, RHO, P0, flags=nat.OUT_PMAG)
    ctx.field_set_medium(cvol, avol, None, model="sampled")
    assert "field_hetero_k" in ctx.field_variant(), ctx.field_variant()
    ctx.field_launch()
    got = np.array([ctx.field_fetch(f, want=("pmag",))["pmag"][vox[f]] for f in range(len(vox))])
    _, b = ctx.bf_solve(foci, C, apod_kind=nat.APOD_MAXANGLE, p0=50.0)
    A, h, dist = ao.arrival(pos_m, foci, avol, origin, spacing, F0, area=area if spreading else None)
    apod = ao.compensate(b, h, mode)
    assert np.abs(a - apod).max() <= 1e-12
    terms = apod * (P0 * area / (C / F0))[None, :] * np.exp(-A) / np.maximum(dist, 0.5 * H)
    for f in range(len(vox)):
        ratio = got[f] / terms[f].sum()
        print(f"focus {vox[f]} ({mode}, spreading={spreading}): |p| {got[f]:.5e} Pa = {ratio:.7f} of the oracle's sum")
        assert abs(ratio - 1) <= 1e-5, ratio
        if mode == "equalize" and spreading:
            act = terms[f][b[f] > 0]
            assert len(act) > 1 and np.abs(act / act[0] - 1).max() <= 1e-12


@pytest.mark.gpu
def test_native_refusals_and_the_state_left_alone(ctx):
    n, h = (13, 11, 16), 1e-3
    origin, spacing, (xs, ys, zs) = _grid(n, h, 4e-3)
    cvol, avol = _skull(xs, ys, zs, third=False)
    _elements(ctx, jitter=False)
    focus = [[0, 0, 15e-3]]
    with pytest.raises(nat.NativeError, match="olx_bf_set_attenuation first"):
        ctx.bf_solve_compensated(focus, C)
    for bad in (-1.0, np.nan, np.inf):
        v = avol.copy(); v[3, 4, 5] = bad
        with pytest.raises(ValueError, match="attenuation"):
            ctx.bf_set_attenuation(v, origin, spacing, n, F0)
    for freq in (0.0, -F0, np.nan, np.inf):
        with pytest.raises(ValueError, match="freq_hz"):
            ctx.bf_set_attenuation(avol, origin, spacing, n, freq)
    with pytest.raises(ValueError, match="grid shape"):
        ctx.bf_set_attenuation(avol[:, :, :-1], origin, spacing, n, F0)
    with pytest.raises(nat.NativeError, match="olx_bf_set_attenuation first"):      # (the refused uploads set nothing)
        ctx.bf_solve_compensated(focus, C)
    ctx.bf_set_attenuation(avol, origin, spacing, n, F0)
    with pytest.raises(nat.NativeError, match="olx_bf_set_medium first"):
        ctx.bf_solve_compensated(focus, C, use_delay_medium=True)
    # a planned heterogeneous field and a delay medium: uploading an attenuation leaves the plan's medium and volumes and the delays as they were
    ctx.bf_set_medium(cvol, origin, spacing, n, C)
    d_before, _ = ctx.bf_solve_medium(focus, C)
    ctx.bf_solve(focus, C)
    ctx.field_plan(origin, spacing, n, F0, C, RHO, P0, flags=nat.OUT_PMAG)
    ctx.field_set_medium(cvol, avol, None, model="sampled")
    ctx.field_launch()
    before = ctx.field_fetch(0, want=("pmag",))["pmag"]
    ctx.bf_set_attenuation(np.full(n, 2.0, dtype=np.float32), origin, spacing, n, 2 * F0)
    assert np.array_equal(ctx.field_fetch(0, want=("pmag",))["pmag"], before)
    ctx.field_launch()
    assert np.array_equal(ctx.field_fetch(0, want=("pmag",))["pmag"], before)
    assert np.array_equal(ctx.bf_solve_medium(focus, C)[0], d_before)
    with pytest.raises(ValueError, match="c_ref"):
        ctx.bf_solve_compensated(focus, 1540.0, use_delay_medium=True)
    with pytest.raises(ValueError, match="share one grid"):
        ctx.bf_set_attenuation(avol, origin, (h, h, 1.5 * h), n, F0)
        ctx.bf_solve_compensated(focus, C, use_delay_medium=True)
    ctx.bf_solve(focus, C)
    assert len(ctx.bf_time(2)) == 2
    ctx.bf_solve_compensated(focus, C)
    with pytest.raises(nat.NativeError, match="olx_bf_time"):
        ctx.bf_time(2)


@pytest.mark.gpu
def test_end_to_end_on_the_skull_protocol():
    proto, setup = _skull_protocol(apod=MediumCompensated(mode="matched"))
    proto.delay_method = StraightRay()
    vol = _volume(setup)
    arr = _array()
    target = ol.Point(position=(0, 0, 20), units="mm")
    sol, _, _ = proto.calc_solution(target, arr, volume=vol, simulate=True, scale=True)
    params = setup.setup_sim_scene(proto.seg_method, volume=vol)
    origin, spacing, n = grid_from_coords(params.coords)
    pos_m, _, area, _, _ = arr.element_table()
    foci = np.array([f.get_position(units="m") for f in sol.foci])
    avol = np.asarray(params["attenuation"].data)
    ref = ao.apodization(pos_m, foci, np.ones((len(foci), len(pos_m))), avol, origin, spacing, proto.pulse.frequency, mode="matched")
    assert ref.max() == 1.0 and ref.min() < 1 - 1e-3
    factor = sol.apodizations.max(axis=1, keepdims=True)            # Solution.scale multiplies each focus' row by one factor <= 1
    print(f"end to end: apodization {ref.min():.4f} .. 1, scale factors {factor.ravel()}, voltage {sol.voltage:.4g}")
    assert (factor > 0).all() and (factor <= 1).all()
    assert np.abs(sol.apodizations - factor * ref).max() <= 1e-12
    cvol = np.asarray(params["sound_speed"].data)
    assert np.abs(sol.delays - mo.delays(pos_m, foci, cvol, origin, spacing, float(params["sound_speed"].attrs["ref_value"]))).max() <= 1e-12
    again = ol.Protocol.from_dict(proto.to_dict())
    assert again.apod_method == proto.apod_method
    sol2, _, _ = again.calc_solution(target, arr, volume=vol, simulate=True, scale=True)
    assert np.array_equal(sol2.apodizations, sol.apodizations) and np.array_equal(sol2.delays, sol.delays)


# ---- the debug library ------------------------------------------------------------------------------------------------------------
def test_bounds_tag_of_the_walk_only_in_the_debug_library():
    """Kernels 1m and 1a are one walk in one translation unit: its bounds words (olx_dbg_bounds_bfmed) cover both."""
    prod = open(os.path.join(LIB, "libolx.so"), "rb").read()
    dbg = open(os.path.join(LIB, "libolx_dbg.so"), "rb").read()
    assert b"olx_dbg_bounds_bfmed" in dbg and b"olx_dbg_bounds_bfmed" not in prod
    assert b"olx_bf_solve_compensated" in dbg and b"olx_bf_solve_compensated" in prod


@pytest.mark.gpu
def test_kernel_1a_stays_inside_its_extents_in_the_debug_library():
    env = dict(os.environ, OLX_LIB_PATH=os.path.join(LIB, "libolx_dbg.so"))
    sel = "matches_oracle or bit_for_bit or one_walk"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", sel, "-p", "no:cacheprovider"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in tail and "failed" not in tail, tail
