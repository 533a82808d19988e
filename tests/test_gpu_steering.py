"""Steering map (kernel 4, olx_steer_map) on the MI355X: full volumes through the C-ABI against the fp64 oracle (tests/steering_oracle.py).

Gates (DESIGN.md section 2 "Steering map"): max |P_gpu - P_ref| <= 1e-5 of the reference's volume maximum (the project's field gate);
n_active bit-equal outside the oracle's excluded mask (voxels with an element on the edge of the fp64 angle decision, relative band 1e-9),
and that mask below 0.1 % of the volume -- asserted, so that it cannot hide a failure.  theta_max = 30 deg: none of the lattice cases below
has a voxel on that cone (45 deg would put 12.7 % of them there).

Identity: P(v) is the CW field of kernel 2 at v when the array is steered to v (olx_bf_solve to v with the same apodization, a CW launch on
the same grid, |p| read at v), within 2e-5 of that launch's volume maximum -- the two 1e-5 gates added."""
import os
import subprocess
import sys

import numpy as np
import pytest

import openlifu_amd as ol
from openlifu_amd import _native as nat
from oracle import bf_oracle as bo
from conftest import synthetic_array
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

# geometry: (array nx, ny, pitch mm, jitter), grid n, spacing mm, z0 mm, x shift mm
MM = {"p7_on_voxels": 2.0 ** -10}      # this case's "mm" is 2^-10 m: voxel and element coordinates are exact in fp64, so w = 0 exactly where they coincide
GEOMS = {"a8": ((8, 8, 3.0, False), (24, 20, 28), 1.0, 5.0, 0.0),
         "b8_plane": ((8, 8, 3.0, False), (25, 21, 27), 1.0, -2.0, 0.0),          # through the element plane, nz = 27: partial quads
         "c16": ((16, 16, 2.0, False), (33, 31, 35), 0.5, 5.0, 0.25),              # 256 elements, nz = 35
         "p7_on_voxels": ((7, 7, 3.0, False), (19, 19, 9), 1.0, -2.0, 0.0),        # every element coincides with a voxel: d = 0, the clamp
         "e3": ((3, 1, 3.0, False), (9, 7, 11), 1.0, 2.0, 0.0),                    # element counts 3 / 100 (64 above): the scalar table's edges
         "e100": ((10, 10, 2.0, False), (9, 7, 11), 1.0, 2.0, 0.0),
         "jit8": ((8, 8, 3.0, True), (24, 20, 28), 1.0, 5.0, 0.0)}                 # jittered positions, tilted normals

# (geometry, apodization, absorption [Np/m], directivity): every instantiation <kind, DIRECTIVITY, ABSORB> of steer_map_k at least once
CASES = [("a8", "uniform", 0.0, False), ("a8", "maxangle30", 0.0, False), ("a8", "piecewise", 5.0, True), ("a8", "piecewise_rad", 0.0, False),
         ("a8", "uniform", 5.0, True),
         ("b8_plane", "uniform", 5.0, False), ("b8_plane", "maxangle30", 0.0, True), ("b8_plane", "piecewise", 0.0, True),
         ("c16", "uniform", 0.0, True), ("c16", "maxangle30", 5.0, False), ("c16", "piecewise", 5.0, False), ("c16", "maxangle30", 5.0, True),
         ("p7_on_voxels", "maxangle30", 0.0, False), ("p7_on_voxels", "piecewise", 5.0, False), ("p7_on_voxels", "uniform", 0.0, False),
         ("e3", "maxangle30", 0.0, False), ("e3", "uniform", 0.0, False), ("e100", "maxangle30", 5.0, False), ("e100", "piecewise", 0.0, True),
         ("jit8", "maxangle30", 0.0, True), ("jit8", "piecewise", 5.0, False), ("jit8", "uniform", 0.0, False)]


def geometry(name):
    (anx, any_, pitch, jitter), n, h, z0, xshift = GEOMS[name]
    mm = MM.get(name, 1e-3)
    pos, ori, size = synthetic_array(anx, any_, pitch, jitter=jitter)
    rot = bo.element_rotations(ori)
    el = dict(pos=pos * mm, nrm=np.ascontiguousarray(rot[:, :, 2]), xaxis=np.ascontiguousarray(rot[:, :, 0]), size=size * mm,
              area=size[:, 0] * size[:, 1] * mm * mm)
    xs = ((np.arange(n[0]) - (n[0] - 1) / 2) * h + xshift) * mm
    ys = (np.arange(n[1]) - (n[1] - 1) / 2) * h * mm
    zs = (z0 + np.arange(n[2]) * h) * mm
    return el, (xs, ys, zs), (h * mm,) * 3, n


_REF = {}


def reference(case):
    """The oracle's (P, n_active, excluded) of a case: computed once, shared by the tests that need it, never written to."""
    if case not in _REF:
        g, a, absorption, directivity = case
        el, (xs, ys, zs), _, _ = geometry(g)
        apod, radians, _ = APODS[a]
        out = so.steering_map(xs, ys, zs, el["pos"], el["nrm"], el["area"], F0, C, P0, apod=apod, radians=radians, absorption=absorption,
                              directivity=(el["xaxis"], el["size"]) if directivity else None)
        for v in out:
            v.setflags(write=False)
        _REF[case] = out
    return _REF[case]


def bind(ctx, el, directivity=False):
    ctx.set_elements(el["pos"], el["nrm"], el["area"])
    if directivity:
        ctx.set_element_apertures(el["xaxis"], el["size"])


def run(ctx, case):
    g, a, absorption, directivity = case
    el, (xs, ys, zs), sp, n = geometry(g)
    bind(ctx, el, directivity)
    kind, p0, p1 = APODS[a][2]
    return ctx.steer_map((xs[0], ys[0], zs[0]), sp, n, F0, C, P0, apod_kind=kind, p0=p0, p1=p1, absorption=absorption, directivity=directivity)


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


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}-a{c[2]:g}-{'dir' if c[3] else 'nodir'}")
def test_steering_map_against_the_oracle(ctx, case):
    pf, na = run(ctx, case)
    check(case, pf, na)


@pytest.mark.gpu
def test_identity_with_the_cw_field_steered_to_the_voxel(ctx):
    case = ("a8", "maxangle30", 0.0, False)
    el, (xs, ys, zs), sp, n = geometry("a8")
    pf, _ = run(ctx, case)
    kind, p0, p1 = APODS["maxangle30"][2]
    rng = np.random.default_rng(11)
    voxels = [(12, 10, 14), (0, 0, 0), (23, 19, 27), (3, 17, 26)] + [tuple(int(rng.integers(0, m)) for m in n) for _ in range(4)]
    for (i, j, k) in voxels:
        ctx.bf_solve(np.array([[xs[i], ys[j], zs[k]]]), C, apod_kind=kind, p0=p0, p1=p1)
        ctx.field_plan((xs[0], ys[0], zs[0]), sp, n, F0, C, RHO, P0, flags=nat.OUT_PMAG)
        ctx.field_launch()
        pm = ctx.field_fetch(0, want=("pmag",))["pmag"]
        d = abs(float(pm[i, j, k]) - float(pf[i, j, k])) / float(pm.max())
        print(f"voxel {(i, j, k)}: |p| {pm[i, j, k]:.6e}, P {pf[i, j, k]:.6e}, difference {d:.3e} of the launch's maximum")
        assert d <= 2e-5, ((i, j, k), d)


@pytest.mark.gpu
def test_a_map_leaves_the_plan_and_the_resident_field_untouched(ctx):
    el, (xs, ys, zs), sp, n = geometry("a8")
    bind(ctx, el, directivity=True)
    ctx.bf_solve(np.array([[1e-3, -2e-3, 20e-3], [0.0, 0.0, 25e-3]]), C, apod_kind=nat.APOD_MAXANGLE, p0=40.0)
    ctx.field_plan((xs[0], ys[0], zs[0]), sp, n, F0, C, RHO, P0)
    ctx.field_launch()
    before = ctx.field_fetch_all()
    variant = ctx.field_variant()
    other = geometry("b8_plane")      # a map on ANOTHER grid, larger than nothing the plan holds
    pf, na = ctx.steer_map((other[1][0][0], other[1][1][0], other[1][2][0]), other[2], other[3], F0, C, P0, apod_kind=nat.APOD_MAXANGLE, p0=30.0,
                           absorption=5.0, directivity=True)
    check(("b8_plane", "maxangle30", 5.0, True), pf, na)
    after = ctx.field_fetch_all()
    assert ctx.field_variant() == variant and variant
    for key in ("pmag", "intensity"):
        assert np.array_equal(before[key].view(np.uint32), after[key].view(np.uint32)), key
    ctx.field_launch()                # the plan and the steering table still launch, to the same bits
    again = ctx.field_fetch_all()
    assert np.array_equal(before["pmag"].view(np.uint32), again["pmag"].view(np.uint32))
    pf2, na2 = ctx.steer_map((other[1][0][0], other[1][1][0], other[1][2][0]), other[2], other[3], F0, C, P0, apod_kind=nat.APOD_MAXANGLE, p0=30.0,
                             absorption=5.0, directivity=True)      # the second call reuses the buffers
    assert np.array_equal(pf.view(np.uint32), pf2.view(np.uint32)) and np.array_equal(na, na2)


@pytest.mark.gpu
def test_missing_state_and_bad_arguments_are_refused(ctx):
    el, (xs, ys, zs), sp, n = geometry("e3")
    args = ((xs[0], ys[0], zs[0]), sp, n, F0, C, P0)
    with pytest.raises(nat.NativeError, match="olx_set_elements"):
        ctx.steer_map(*args)
    bind(ctx, el)
    with pytest.raises(nat.NativeError, match="olx_set_element_apertures"):
        ctx.steer_map(*args, directivity=True)
    with pytest.raises(nat.NativeError, match="olx_steer_map"):
        ctx.steer_time(1)
    with pytest.raises(ValueError, match="rolloff"):
        ctx.steer_map(*args, apod_kind=nat.APOD_PIECEWISE, p0=20.0, p1=40.0)
    with pytest.raises(ValueError, match="absorption"):
        ctx.steer_map(*args, absorption=-1.0)
    pf, na = ctx.steer_map(*args)
    assert np.all(na == 3) and np.all(pf > 0)
    assert ctx.steer_time(2).shape == (2,)


@pytest.mark.gpu
def test_python_interface_against_the_oracle():
    arr = ol.Transducer.gen_matrix_array(nx=8, ny=8, pitch=3, kerf=0.3, units="mm", sensitivity=2.0)
    arr.frequency = F0
    setup = ol.SimSetup(spacing=1.0, x_extent=(-6, 6), y_extent=(-5, 5), z_extent=(5, 22))
    proto = ol.Protocol(pulse=ol.Pulse(frequency=F0, amplitude=0.5, duration=2e-5), sim_setup=setup, apod_method=ol.apod_methods.MaxAngle(max_angle=30.0))
    from openlifu_amd.sim.field import _np_per_m
    from openlifu_amd.engine import get_engine
    params = setup.setup_sim_scene(ol.seg.seg_methods.UniformWater())
    alpha = _np_per_m(params["attenuation"].attrs["ref_value"], F0)      # the scene's uniform attenuation enters as exp(-alpha d)
    sm = proto.calc_steering_map(arr)
    coords = setup.get_coords()
    xs, ys, zs = (np.asarray(coords[d].data, dtype=np.float64) * 1e-3 for d in ("x", "y", "z"))
    pos, nrm, area, _, _ = arr.element_table()
    P, n_ref, excl = so.steering_map(xs, ys, zs, pos, nrm, area, F0, C, 1.0, apod=("maxangle", 30.0, 0.0), absorption=alpha)
    assert excl.mean() < MAX_EXCLUDED
    pf = np.asarray(sm.dataset["focal_pressure"].data)
    assert pf.shape == P.shape and np.abs(pf - P).max() / P.max() <= TOL
    assert np.array_equal(np.asarray(sm.dataset["n_active"].data)[~excl], n_ref[~excl])
    assert sm.reference_index == tuple(int(v) for v in np.unravel_index(np.argmax(pf), pf.shape))
    g = np.asarray(sm.dataset["steering_gain_db"].data)
    assert g.max() == 0.0 and np.array_equal(sm.envelope(-6.0), g >= -6.0)
    tcs = sm.to_target_constraints(-6.0)
    assert [t.dim for t in tcs] == ["x", "y", "z"] and all(t.units == "mm" and t.min <= t.max for t in tcs)
    # the module function, with attenuation and directivity; reference = a point
    sm2 = ol.plan.calc_steering_map(arr, params, apod_method=ol.apod_methods.PiecewiseLinear(zero_angle=40.0, rolloff_angle=20.0),
                                    amplitude=0.5, directivity=True, reference=(0.0, 0.0, 15.0))
    assert sm2.reference_index == (6, 5, 10) and np.asarray(sm2.dataset["steering_gain_db"].data)[6, 5, 10] == 0.0
    xaxis, size = arr.element_apertures()
    P2, _, _ = so.steering_map(xs, ys, zs, pos, nrm, area, F0, C, 1.0, apod=("piecewise", 40.0, 20.0), absorption=alpha, directivity=(xaxis, size))
    assert np.abs(np.asarray(sm2.dataset["focal_pressure"].data) - P2).max() / P2.max() <= TOL
    eng = get_engine()
    eng.ctx.comm_transport = lambda: "rccl"       # a context that belongs to a communicator is refused
    try:
        with pytest.raises(NotImplementedError, match="communicator"):
            proto.calc_steering_map(arr)
    finally:
        del eng.ctx.comm_transport


@pytest.mark.gpu
def test_the_map_kernel_stays_inside_its_extents_in_the_debug_library():
    code = r"""
import sys
for p in (%r, %r, %r):
    sys.path.insert(0, p)
import numpy as np
from openlifu_amd import _native as nat
import test_gpu_steering as t
ctx = nat.Context(0)
case = ("b8_plane", "piecewise", 0.0, True)
pf, na = t.run(ctx, case)
try:
    ctx.sync()
except nat.NativeError as e:
    print("REPORTED:", e)
    sys.exit(0 if ("outside their extent" in str(e) and "k_steer" in str(e)) else 3)
t.check(case, pf, na)
sys.exit(4)
""" % (ROOT, os.path.join(ROOT, "openlifu-python_amd"), os.path.join(ROOT, "tests"))
    env = dict(os.environ, OLX_LIB_PATH=os.path.join(LIB, "libolx_dbg.so"))
    env.pop("OLX_DEBUG_BOUNDS_SELFTEST", None)
    ok = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert ok.returncode == 4, (ok.returncode, (ok.stdout + ok.stderr)[-2000:])          # clean run: nothing to report, values right
    bad = subprocess.run([sys.executable, "-c", code], env=dict(env, OLX_DEBUG_BOUNDS_SELFTEST="1"), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert bad.returncode == 0 and "REPORTED:" in bad.stdout, (bad.returncode, (bad.stdout + bad.stderr)[-2000:])
