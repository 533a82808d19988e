"""Steering map through a heterogeneous medium (kernel 4h, olx_steer_map_medium) on the MI355X: full volumes through the C-ABI against the fp64
oracle (tests/steering_medium_oracle.py).

Gates (DESIGN.md section 2 "Steering map through a medium"), all the project's own: max |P_gpu - P_ref| <= 1e-5 of the reference's volume maximum
(the field gate; kernel 2h measures 0.9 - 1.9e-6 with the same stencil arithmetic); n_active bit-equal outside the oracle's excluded mask, and
that mask below 0.1 % of the volume -- asserted.  Geometries: kernel 4's own (tests/test_gpu_steering.py), restated here; with the 30 deg cone
none of them has a voxel on a decision edge.

Phantom: a slab on planes 8 .. 15 with c = 2800 m/s and 8 dB/cm/MHz^0.9 whose thickness and values vary with x and y; for b8_plane a second region on
planes 0 .. 1 BELOW the array (the klast branch) and a non-zero medium on plane 2, the element plane, which must never count as a crossing; the
grids of 11 planes also carry a thin layer on planes 3 .. 4 (their slab is cut off at plane 10).

Identities: with both volumes NULL the map is kernel 4's with absorption 0; P(v) is the |p| at v of the sampled heterogeneous field (kernel 2h)
when the array is steered to v with the matching resident steering table, within 2e-5 of that launch's maximum (the two 1e-5 gates added)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import openlifu_amd as ol
from openlifu_amd import _native as nat
from openlifu_amd.engine import grid_from_coords
from openlifu_amd.util import dataset as ds
from oracle import bf_oracle as bo
from conftest import synthetic_array
import steering_medium_oracle as smo
import steering_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "openlifu-python_amd", "lib")
F0, C, RHO, P0 = 400e3, 1500.0, 1000.0, 1e5
TOL, MAX_EXCLUDED = 1e-5, 1e-3

APODS = {"uniform": (("uniform", 0.8, 0.0), False, (nat.APOD_UNIFORM, 0.8, 0.0)),
         "maxangle30": (("maxangle", 30.0, 0.0), False, (nat.APOD_MAXANGLE, 30.0, 0.0)),
         "piecewise": (("piecewise", 40.0, 20.0), False, (nat.APOD_PIECEWISE, 40.0, 20.0)),
         "piecewise_rad": (("piecewise", np.radians(40.0), np.radians(20.0)), True,
                           (nat.APOD_PIECEWISE | 0x10, np.radians(40.0), np.radians(20.0)))}

# geometry: (array nx, ny, pitch mm, jitter), grid n, spacing mm, z0 mm
GEOMS = {"a8": ((8, 8, 3.0, False), (24, 20, 28), 1.0, 5.0),
         "b8_plane": ((8, 8, 3.0, False), (25, 21, 27), 1.0, -2.0),        # through the element plane (plane 2), odd nz: partial quads
         "jit8": ((8, 8, 3.0, True), (24, 20, 28), 1.0, 5.0),               # jittered positions, tilted normals
         "e3": ((3, 1, 3.0, False), (9, 7, 11), 1.0, 2.0),                  # element counts 3 / 100: the scalar tables' edges
         "e100": ((10, 10, 2.0, False), (9, 7, 11), 1.0, 2.0),
         "line": ((3, 1, 3.0, False), (1, 7, 11), 1.0, 2.0)}                # a single-voxel axis: border extension, 7 of 8 tile rows idle


def _cases():
    """(geometry, apodization, comp, spreading, delays, directivity, volumes): every instantiation <KIND, COMP, PHASE, DIRECTIVITY> of
    steer_map_med_k once, spreading on and off in each comp mode, then the element counts, the single-voxel axis and the volume combinations."""
    out, q = [], 0
    for kind in ("uniform", "maxangle30", "piecewise"):
        for comp in (None, "equalize", "matched"):
            for delays in ("straight_ray", "direct"):
                out.append(("a8", kind, comp, q % 2 == 1, delays, False, "both"))
                out.append(("b8_plane" if q % 2 == 0 else "jit8", kind, comp, q % 2 == 0, delays, True, "both"))
                q += 1
    out += [("b8_plane", "maxangle30", "equalize", False, "straight_ray", False, "both"), ("b8_plane", "piecewise_rad", None, False, "direct", False, "both"),
            ("jit8", "piecewise", "matched", True, "straight_ray", False, "both"),
            ("e3", "maxangle30", "matched", False, "direct", False, "both"), ("e3", "uniform", "equalize", True, "straight_ray", False, "both"),
            ("e100", "piecewise", "equalize", True, "straight_ray", True, "both"), ("e100", "uniform", None, False, "direct", False, "both"),
            ("line", "maxangle30", "matched", True, "direct", False, "both"), ("line", "uniform", "equalize", False, "straight_ray", False, "both"),
            ("a8", "maxangle30", "matched", False, "direct", False, "ss"), ("a8", "maxangle30", "matched", False, "direct", False, "att"),
            ("a8", "maxangle30", "matched", False, "direct", False, "none"), ("a8", "uniform", "equalize", True, "straight_ray", False, "ss"),
            ("a8", "piecewise", None, False, "straight_ray", False, "att"), ("a8", "uniform", None, False, "straight_ray", False, "none")]
    return out


CASES = _cases()


def geometry(name):
    (anx, any_, pitch, jitter), n, h, z0 = GEOMS[name]
    mm = 1e-3
    pos, ori, size = synthetic_array(anx, any_, pitch, jitter=jitter)
    rot = bo.element_rotations(ori)
    el = dict(pos=pos * mm, nrm=np.ascontiguousarray(rot[:, :, 2]), xaxis=np.ascontiguousarray(rot[:, :, 0]), size=size * mm,
              area=size[:, 0] * size[:, 1] * mm * mm)
    origin = (-(n[0] - 1) / 2 * h * mm, -(n[1] - 1) / 2 * h * mm, z0 * mm)
    return el, origin, (h * mm,) * 3, n


def phantom(name, volumes="both"):
    """(sound speed, attenuation) float32 [nx, ny, nz], or None for a volume the case leaves out."""
    n = GEOMS[name][1]
    I, J, K = np.meshgrid(*(np.arange(m) for m in n), indexing="ij")
    ss = np.full(n, C, dtype=np.float32)
    att = np.zeros(n, dtype=np.float32)
    slab = (K >= 8 + (I + J) % 2) & (K <= 15 - (I // 3) % 2)
    ss[slab] = (2800.0 * (1 + 0.04 * np.sin(0.7 * I + 0.4 * J)))[slab]
    att[slab] = (8.0 * (1 + 0.2 * np.cos(0.5 * I - 0.3 * J)))[slab]
    if name == "b8_plane":
        below = K <= 1
        ss[below] = (1700.0 + 10.0 * I)[below]; att[below] = (2.0 + 0.1 * J)[below]
        ss[K == 2] = (1600.0 + 5.0 * J)[K == 2]; att[K == 2] = (1.0 + 0.05 * I)[K == 2]
    if n[2] == 11:
        thin = (K >= 3) & (K <= 4 - J % 2)
        ss[thin] = 2000.0; att[thin] = (4.0 + 0.3 * J)[thin]
    return (ss if volumes in ("both", "ss") else None), (att if volumes in ("both", "att") else None)


_SUMS, _REF = {}, {}


def sums(name, volumes):
    """The oracle's ray sums (A, E) of a geometry and phantom: computed once, shared by every mode, never written to."""
    if (name, volumes) not in _SUMS:
        el, origin, sp, n = geometry(name)
        ss, att = phantom(name, volumes)
        out = smo.medium_sums(origin, sp, n, el["pos"], F0, C, ss, att)
        for v in out:
            v.setflags(write=False)
        _SUMS[(name, volumes)] = out
    return _SUMS[(name, volumes)]


def reference(case):
    if case not in _REF:
        g, a, comp, spreading, delays, directivity, volumes = case
        el, origin, sp, n = geometry(g)
        apod, radians, _ = APODS[a]
        out = smo.steering_map_medium(origin, sp, n, el["pos"], el["nrm"], el["area"], F0, C, P0, apod=apod, radians=radians, comp=comp,
                                      spreading=spreading, delays=delays, directivity=(el["xaxis"], el["size"]) if directivity else None,
                                      sums=sums(g, volumes))
        for v in out:
            v.setflags(write=False)
        _REF[case] = out
    return _REF[case]


def bind(ctx, el, directivity=False):
    ctx.set_elements(el["pos"], el["nrm"], el["area"])
    if directivity:
        ctx.set_element_apertures(el["xaxis"], el["size"])


def run(ctx, case):
    g, a, comp, spreading, delays, directivity, volumes = case
    el, origin, sp, n = geometry(g)
    bind(ctx, el, directivity)
    kind, p0, p1 = APODS[a][2]
    ss, att = phantom(g, volumes)
    return ctx.steer_map_medium(origin, sp, n, F0, C, P0, apod_kind=kind, p0=p0, p1=p1, sound_speed=ss, attenuation=att, comp=comp,
                                spreading=spreading, delays=delays, directivity=directivity)


def check(case, pf, na):
    P, n_ref, excl = reference(case)
    err = np.abs(pf.astype(np.float64) - P).max() / P.max()
    share = excl.mean()
    bad = int(np.count_nonzero((na != n_ref) & ~excl))
    print(f"{case}: max |dP| / max P = {err:.3e}, excluded {share:.4%}, n_active mismatches outside the mask {bad}, max P = {P.max():.4e}")
    assert share < MAX_EXCLUDED, share
    assert pf.dtype == np.float32 and na.dtype == np.int32 and pf.shape == P.shape
    assert err <= TOL, err
    assert bad == 0, bad


def case_id(c):
    return f"{c[0]}-{c[1]}-{c[2] or 'plain'}{'-spread' if c[3] else ''}-{c[4]}-{'dir' if c[5] else 'nodir'}-{c[6]}"


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_medium_map_against_the_oracle(ctx, case):
    pf, na = run(ctx, case)
    check(case, pf, na)


@pytest.mark.gpu
def test_identity_with_kernel_4_when_both_volumes_are_null(ctx):
    for g, a, delays, directivity in (("a8", "maxangle30", "straight_ray", False), ("b8_plane", "piecewise", "direct", True),
                                      ("jit8", "uniform", "direct", False)):
        el, origin, sp, n = geometry(g)
        bind(ctx, el, directivity)
        kind, p0, p1 = APODS[a][2]
        ref, n_ref = ctx.steer_map(origin, sp, n, F0, C, P0, apod_kind=kind, p0=p0, p1=p1, absorption=0.0, directivity=directivity)
        pf, na = ctx.steer_map_medium(origin, sp, n, F0, C, P0, apod_kind=kind, p0=p0, p1=p1, delays=delays, directivity=directivity)
        err = np.abs(pf.astype(np.float64) - ref).max() / ref.max()
        print(f"{g} {a} {delays}: max |P_4h - P_4| / max = {err:.3e}")
        assert err <= 1e-5 and np.array_equal(na, n_ref)


FIELD_MODES = {"straightray_matched": ("maxangle30", "matched", "straight_ray"), "straightray_maxangle": ("maxangle30", None, "straight_ray"),
               "direct_uniform": ("uniform", None, "direct")}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(FIELD_MODES))
def test_identity_with_the_sampled_field_steered_to_the_voxel(ctx, mode):
    a, comp, delays = FIELD_MODES[mode]
    el, origin, sp, n = geometry("a8")
    ss, att = phantom("a8")
    xs, ys, zs = smo.grid_axes(origin, sp, n)
    case = ("a8", a, comp, False, delays, False, "both")
    pf, _ = run(ctx, case)
    kind, p0, p1 = APODS[a][2]
    rng = np.random.default_rng(11)
    voxels = [(12, 10, 14), (0, 0, 0), (23, 19, 27), (3, 17, 26)] + [tuple(int(rng.integers(0, m)) for m in n) for _ in range(4)]
    for (i, j, k) in voxels:
        r = np.array([[xs[i], ys[j], zs[k]]])
        assert np.linalg.norm(r - el["pos"], axis=1).min() >= 3e-3
        if mode == "straightray_matched":
            ctx.bf_set_medium(ss, origin, sp, n, C)
            ctx.bf_set_attenuation(att, origin, sp, n, F0)
            ctx.bf_solve_compensated(r, C, apod_kind=kind, p0=p0, p1=p1, mode="matched", use_delay_medium=True)
        elif mode == "straightray_maxangle":
            ctx.bf_set_medium(ss, origin, sp, n, C)
            ctx.bf_solve_medium(r, C, apod_kind=kind, p0=p0, p1=p1)
        else:
            ctx.bf_solve(r, C, apod_kind=kind, p0=p0, p1=p1)
        ctx.field_plan(origin, sp, n, F0, C, RHO, P0, flags=nat.OUT_PMAG)
        ctx.field_set_medium(ss, att, None, model="sampled")
        ctx.field_launch()
        pm = ctx.field_fetch(0, want=("pmag",))["pmag"]
        d = abs(float(pm[i, j, k]) - float(pf[i, j, k])) / float(pm.max())
        print(f"{mode} voxel {(i, j, k)}: |p| {pm[i, j, k]:.6e}, P {pf[i, j, k]:.6e}, difference {d:.3e} of the launch's maximum")
        assert d <= 2e-5, ((i, j, k), d)


@pytest.mark.gpu
def test_a_map_leaves_the_plan_its_medium_the_steering_table_and_the_beamformer_media_untouched(ctx):
    el, origin, sp, n = geometry("a8")
    ss, att = phantom("a8")
    bind(ctx, el, directivity=True)
    foci = np.array([[1e-3, -2e-3, 25e-3], [0.0, 0.0, 30e-3]])
    ctx.bf_set_medium(ss, origin, sp, n, C)
    ctx.bf_set_attenuation(att, origin, sp, n, F0)
    d0, a0 = ctx.bf_solve_compensated(foci, C, apod_kind=nat.APOD_MAXANGLE, p0=40.0, mode="equalize", use_delay_medium=True)
    ctx.field_plan(origin, sp, n, F0, C, RHO, P0)
    ctx.field_set_medium(ss, att, None, model="sampled")
    ctx.field_launch()
    before = ctx.field_fetch_all()
    variant = ctx.field_variant()
    case = ("b8_plane", "maxangle30", "matched", True, "direct", True, "both")      # a map on ANOTHER grid, with another medium
    _, o_origin, o_sp, o_n = geometry("b8_plane")
    o_ss, o_att = phantom("b8_plane")
    args = dict(apod_kind=nat.APOD_MAXANGLE, p0=30.0, sound_speed=o_ss, attenuation=o_att, comp="matched", spreading=True, delays="direct", directivity=True)
    pf, na = ctx.steer_map_medium(o_origin, o_sp, o_n, F0, C, P0, **args)
    check(case, pf, na)
    after = ctx.field_fetch_all()
    assert ctx.field_variant() == variant and variant
    for key in ("pmag", "intensity"):
        assert np.array_equal(before[key].view(np.uint32), after[key].view(np.uint32)), key
    ctx.field_launch()                # the plan, its medium and the steering table still launch, to the same bits
    again = ctx.field_fetch_all()
    assert np.array_equal(before["pmag"].view(np.uint32), again["pmag"].view(np.uint32))
    d1, a1 = ctx.bf_solve_compensated(foci, C, apod_kind=nat.APOD_MAXANGLE, p0=40.0, mode="equalize", use_delay_medium=True)      # the 1m / 1a media
    assert np.array_equal(d0.view(np.uint64), d1.view(np.uint64)) and np.array_equal(a0.view(np.uint64), a1.view(np.uint64))
    pf2, na2 = ctx.steer_map_medium(o_origin, o_sp, o_n, F0, C, P0, **args)      # the second call reuses the buffers
    assert np.array_equal(pf.view(np.uint32), pf2.view(np.uint32)) and np.array_equal(na, na2)
    ms = ctx.steer_time(2)            # olx_steer_time repeats the last map of either kind
    assert ms.shape == (2,) and np.all(ms > 0)


def raw_call(ctx, origin, sp, n, comp, delays):
    g = nat.OlxGrid()
    for a in range(3):
        g.origin[a] = origin[a]; g.spacing[a] = sp[a]; g.n[a] = n[a]
    pf = np.empty(n, dtype=np.float32)
    rc = ctx._lib.olx_steer_map_medium(ctx._h, ctypes.byref(g), F0, C, P0, nat.APOD_UNIFORM, 1.0, 0.0, None, None, comp, 0, delays, 0, nat._fptr(pf), None)
    return rc, ctx._lib.olx_last_error(ctx._h).decode()


@pytest.mark.gpu
def test_missing_state_and_bad_arguments_are_refused(ctx):
    el, origin, sp, n = geometry("e3")
    ss, att = phantom("e3")
    args = (origin, sp, n, F0, C, P0)
    with pytest.raises(nat.NativeError, match="olx_set_elements"):
        ctx.steer_map_medium(*args, sound_speed=ss, attenuation=att)
    bind(ctx, el)
    with pytest.raises(nat.NativeError, match="olx_set_element_apertures"):
        ctx.steer_map_medium(*args, directivity=True)
    with pytest.raises(ValueError, match="spacing"):
        ctx.steer_map_medium(origin, (1e-3, 0.0, 1e-3), n, F0, C, P0)
    with pytest.raises(ValueError, match="grid sizes"):
        ctx.steer_map_medium(origin, sp, (9, 0, 11), F0, C, P0)
    for f, c in ((0.0, C), (np.inf, C), (F0, -1.0), (F0, np.nan)):
        with pytest.raises(ValueError, match="freq and c_ref"):
            ctx.steer_map_medium(origin, sp, n, f, c, P0)
    for bad in (0.0, -1500.0, np.nan, np.inf):
        v = ss.copy(); v[4, 3, 5] = bad
        with pytest.raises(ValueError, match="sound speed"):
            ctx.steer_map_medium(*args, sound_speed=v)
    for bad in (-0.5, np.nan, np.inf):
        v = att.copy(); v[4, 3, 5] = bad
        with pytest.raises(ValueError, match="attenuation"):
            ctx.steer_map_medium(*args, attenuation=v)
    with pytest.raises(ValueError, match="rolloff"):
        ctx.steer_map_medium(*args, apod_kind=nat.APOD_PIECEWISE, p0=20.0, p1=40.0)
    with pytest.raises(ValueError, match="comp"):
        ctx.steer_map_medium(*args, comp="flatten")
    with pytest.raises(ValueError, match="delays"):
        ctx.steer_map_medium(*args, delays="marched")
    rc, msg = raw_call(ctx, origin, sp, n, 7, 0)          # ... and the C-ABI's own refusals of the two selectors
    assert rc == nat.OLX_EINVAL and "unknown comp 7" in msg
    rc, msg = raw_call(ctx, origin, sp, n, -1, 2)
    assert rc == nat.OLX_EINVAL and "unknown delays 2" in msg
    with pytest.raises(nat.NativeError, match="olx_steer_map"):
        ctx.steer_time(1)             # none of the refusals left a map behind
    pf, na = ctx.steer_map_medium(*args, sound_speed=ss, attenuation=att, comp="matched", delays="direct")
    assert np.all(na == 3) and np.all(pf > 0)
    assert ctx.steer_time(2).shape == (2,)


@pytest.mark.gpu
def test_python_interface_against_the_oracle():
    arr = ol.Transducer.gen_matrix_array(nx=8, ny=8, pitch=3, kerf=0.3, units="mm", sensitivity=2.0)
    arr.frequency = F0
    setup = ol.SimSetup(spacing=1.0, x_extent=(-6, 6), y_extent=(-5, 5), z_extent=(5, 22))
    params = setup.setup_sim_scene(ol.seg.seg_methods.UniformWater())
    coords = setup.get_coords()
    origin, sp, n = grid_from_coords(coords)
    n = tuple(int(v) for v in n)
    I, J, K = np.meshgrid(*(np.arange(m) for m in n), indexing="ij")
    slab = (K >= 6 + (I + J) % 2) & (K <= 11 - (I // 3) % 2)
    ss = np.full(n, C, dtype=np.float32); ss[slab] = (2800.0 * (1 + 0.04 * np.sin(0.7 * I + 0.4 * J)))[slab]
    att = np.zeros(n, dtype=np.float32); att[slab] = (8.0 * (1 + 0.2 * np.cos(0.5 * I - 0.3 * J)))[slab]
    for key, vol in (("sound_speed", ss), ("attenuation", att)):
        params[key] = ds.make_dataarray(vol, coords=params.coords, dims=list(params.coords.keys()), name=key, attrs=dict(params[key].attrs))
    assert float(params["sound_speed"].attrs["ref_value"]) == C
    proto = ol.Protocol(pulse=ol.Pulse(frequency=F0, amplitude=0.5, duration=2e-5), sim_setup=setup,
                        apod_method=ol.apod_methods.MediumCompensated(mode="matched"), delay_method=ol.delay_methods.StraightRay())
    with pytest.raises(NotImplementedError):
        proto.calc_steering_map(arr, params)          # the default mode still refuses
    sm = proto.calc_steering_map(arr, params, medium_model="straight_ray")
    pos, nrm, area, _, _ = arr.element_table()
    P, n_ref, excl = smo.steering_map_medium(origin, sp, n, pos, nrm, area, F0, C, 1.0, apod=("uniform", 1.0, 0.0), sound_speed=ss, attenuation=att,
                                             comp="matched")
    pf = np.asarray(sm.dataset["focal_pressure"].data)
    err = np.abs(pf - P).max() / P.max()
    print(f"Protocol.calc_steering_map(medium_model='straight_ray'): max |dP| / max P = {err:.3e}")
    assert pf.shape == P.shape and err <= TOL and not excl.any()
    assert np.array_equal(np.asarray(sm.dataset["n_active"].data), n_ref)
    xs, ys, zs = smo.grid_axes(origin, sp, n)
    water, _, _ = so.steering_map(xs, ys, zs, pos, nrm, area, F0, C, 1.0)      # p0 = amplitude 0.5 x sensitivity 2
    mg = np.asarray(sm.dataset["medium_gain_db"].data)
    assert np.abs(mg - 20 * np.log10(pf / water)).max() <= 1e-3 and mg.max() <= 1e-3 and mg.min() < -1.0       # the slab costs pressure behind it
    assert sm.reference_index == tuple(int(v) for v in np.unravel_index(np.argmax(pf), pf.shape))
    g = np.asarray(sm.dataset["steering_gain_db"].data)
    assert g.max() == 0.0 and np.array_equal(sm.envelope(-6.0), g >= -6.0)
    tcs = sm.to_target_constraints(-6.0)
    assert [t.dim for t in tcs] == ["x", "y", "z"] and all(t.units == "mm" and t.min <= t.max for t in tcs)
    direct = ol.plan.calc_steering_map(arr, params, apod_method=ol.apod_methods.MaxAngle(max_angle=30.0), amplitude=0.5,
                                       medium_model="straight_ray", delay_method=ol.delay_methods.Direct())
    P2, _, ex2 = smo.steering_map_medium(origin, sp, n, pos, nrm, area, F0, C, 1.0, apod=("maxangle", 30.0, 0.0), sound_speed=ss, attenuation=att,
                                         delays="direct")
    assert ex2.mean() < MAX_EXCLUDED and np.abs(np.asarray(direct.dataset["focal_pressure"].data) - P2).max() / P2.max() <= TOL


@pytest.mark.gpu
def test_the_map_kernel_stays_inside_its_extents_in_the_debug_library():
    code = r"""
import sys
for p in (%r, %r, %r):
    sys.path.insert(0, p)
import numpy as np
from openlifu_amd import _native as nat
import test_gpu_steering_medium as t
ctx = nat.Context(0)
case = ("b8_plane", "piecewise", "matched", True, "direct", True, "both")
pf, na = t.run(ctx, case)
try:
    ctx.sync()
except nat.NativeError as e:
    print("REPORTED:", e)
    sys.exit(0 if ("outside their extent" in str(e) and "k_steer_med" in str(e)) else 3)
t.check(case, pf, na)
sys.exit(4)
""" % (ROOT, os.path.join(ROOT, "openlifu-python_amd"), os.path.join(ROOT, "tests"))
    env = dict(os.environ, OLX_LIB_PATH=os.path.join(LIB, "libolx_dbg.so"))
    env.pop("OLX_DEBUG_BOUNDS_SELFTEST", None)
    ok = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert ok.returncode == 4, (ok.returncode, (ok.stdout + ok.stderr)[-2000:])          # clean run: nothing to report, values right
    bad = subprocess.run([sys.executable, "-c", code], env=dict(env, OLX_DEBUG_BOUNDS_SELFTEST="1"), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert bad.returncode == 0 and "REPORTED:" in bad.stdout, (bad.returncode, (bad.stdout + bad.stderr)[-2000:])
