"""Steering map on the host: the fp64 oracle (tests/steering_oracle.py) against closed forms of the definition (DESIGN.md section 2
"Steering map"), the gain / envelope / target-constraint logic of ``SteeringMap`` on a synthetic volume, and the refusals of
``calc_steering_map`` -- all raised before anything touches the device."""
import numpy as np
import pytest

import openlifu_amd as ol
from openlifu_amd.plan import SteeringMap, calc_steering_map
from openlifu_amd.plan.steering import nearest_voxel, steering_gain_db
from openlifu_amd.seg.material import Material
from openlifu_amd.util import dataset as ds
from oracle.field_oracle import piston_directivity
import steering_oracle as so

F0, C, P0 = 400e3, 1500.0, 1e5
LAM = C / F0
S = 4e-6
ONE = dict(pos_m=np.zeros((1, 3)), normal=np.array([[0.0, 0.0, 1.0]]), area_m2=np.array([S]))


def axes(n, h, origin):
    return tuple(origin[a] + np.arange(n[a]) * h for a in range(3))


def test_one_element_on_its_axis():
    zs = 5e-3 + np.arange(6) * 1e-3
    P, na, ex = so.steering_map([0.0], [0.0], zs, freq=F0, c=C, p0_pa=P0, **ONE)
    assert np.allclose(P[0, 0], P0 * S / (LAM * zs), rtol=1e-14) and np.all(na == 1) and not ex.any()


def test_clamp_below_dmin_and_theta_zero_at_d_zero():
    h = 1e-3
    xs, ys, zs = axes((3, 3, 3), h, (-h, -h, -h))          # the centre voxel IS the element
    zs = zs * 0.2                                            # z step 0.2 mm: dmin = 0.1 mm, the voxels above / below sit at d = 0.2 mm
    P, na, _ = so.steering_map(xs, ys, zs, freq=F0, c=C, p0_pa=P0, apod=("maxangle", 30.0, 0.0), **ONE)
    assert P[1, 1, 1] == pytest.approx(P0 * S / (LAM * 1e-4), rel=1e-14) and na[1, 1, 1] == 1       # d = 0: clamped, theta = 0 passes
    assert P[1, 1, 2] == pytest.approx(P0 * S / (LAM * 2e-4), rel=1e-12)
    P2, _, _ = so.steering_map(xs, ys, [0.0, 0.04e-3], freq=F0, c=C, p0_pa=P0, **ONE)                   # z step 0.04 mm: dmin = 0.02 mm
    assert P2[1, 1, 1] == pytest.approx(P0 * S / (LAM * 0.04e-3), rel=1e-12) and P2[1, 1, 0] == pytest.approx(P0 * S / (LAM * 0.02e-3), rel=1e-12)       # d = 0 -> dmin
    Pw, naw, _ = so.steering_map(xs, ys, zs, freq=F0, c=C, p0_pa=P0, apod=("piecewise", 40.0, 20.0), **ONE)
    assert naw[1, 1, 1] == 1 and Pw[1, 1, 1] == pytest.approx(P[1, 1, 1], rel=1e-14)                   # theta = 0 -> a = 1


def test_maxangle_cone_of_one_element():
    xs, ys, zs = axes((41, 1, 21), 0.5e-3, (-10e-3, 0.0, 0.25e-3))
    P, na, ex = so.steering_map(xs, ys, zs, freq=F0, c=C, p0_pa=P0, apod=("maxangle", 30.0, 0.0), **ONE)
    X, Z = np.meshgrid(xs, zs, indexing="ij")
    inside = np.degrees(np.arctan2(np.abs(X), Z)) <= 30.0
    assert np.array_equal((na[:, 0, :] == 1)[~ex[:, 0, :]], inside[~ex[:, 0, :]]) and ex.mean() < 0.01
    assert np.all(P[:, 0, :][~inside & ~ex[:, 0, :]] == 0) and np.all(P[:, 0, :][inside] > 0)
    Pr, nar, _ = so.steering_map(xs, ys, zs, freq=F0, c=C, p0_pa=P0, apod=("maxangle", np.pi / 6, 0.0), radians=True, **ONE)
    assert np.array_equal(nar[~ex], na[~ex])
    Pa, naa, exa = so.steering_map(xs, ys, zs, freq=F0, c=C, p0_pa=P0, apod=("maxangle", 90.0, 0.0), **ONE)
    assert np.all(naa == 1) and not exa.any()                                                          # >= 90 deg passes everything


def test_piecewise_linear_weights():
    xs, ys, zs = axes((1, 1, 1), 1e-3, (10e-3 * np.tan(np.radians(30.0)), 0.0, 10e-3))              # theta = 30 deg
    P, na, _ = so.steering_map(xs, ys, zs, freq=F0, c=C, p0_pa=P0, apod=("piecewise", 40.0, 20.0), **ONE)
    d = np.hypot(xs[0], zs[0])
    assert P[0, 0, 0] == pytest.approx(0.5 * P0 * S / (LAM * d), rel=1e-9) and na[0, 0, 0] == 1


def test_absorption():
    zs = 5e-3 + np.arange(6) * 1e-3
    P0v, _, _ = so.steering_map([0.0], [0.0], zs, freq=F0, c=C, p0_pa=P0, **ONE)
    Pa, _, _ = so.steering_map([0.0], [0.0], zs, freq=F0, c=C, p0_pa=P0, absorption=5.0, **ONE)
    assert np.allclose(Pa / P0v, np.exp(-5.0 * zs)[None, None, :], rtol=1e-14)


def test_directivity_is_the_field_oracles_piston_factor():
    rng = np.random.default_rng(5)
    pos = rng.uniform(-5e-3, 5e-3, (4, 3)); pos[:, 2] = 0
    nrm = np.tile([0.0, 0.0, 1.0], (4, 1)); xaxis = np.tile([1.0, 0.0, 0.0], (4, 1)); size = np.tile([2.7e-3, 1.9e-3], (4, 1))
    area = size[:, 0] * size[:, 1]
    xs, ys, zs = axes((5, 4, 3), 2e-3, (-4e-3, -3e-3, 8e-3))
    Pd, _, _ = so.steering_map(xs, ys, zs, pos, nrm, area, F0, C, P0, directivity=(xaxis, size))
    pts = np.stack(np.meshgrid(xs, ys, zs, indexing="ij"), axis=-1).reshape(-1, 3)
    w = pts[:, None, :] - pos[None, :, :]
    d = np.sqrt((w * w).sum(axis=2))
    ref = (P0 * area[None, :] / (LAM * d) * piston_directivity(w, d, xaxis, nrm, size, F0, C)).sum(axis=1)
    assert np.allclose(Pd.ravel(), ref, rtol=1e-13)


# ---- SteeringMap on a synthetic volume --------------------------------------------------------------------------------
def synthetic_map(reference=None):
    vec = {"x": np.arange(-4.0, 5.0), "y": np.arange(-3.0, 4.0), "z": 10.0 + 2.0 * np.arange(6)}
    coords = ds.make_coords(vec, {d: {"units": "mm", "long_name": n} for d, n in zip("xyz", ("Lateral", "Elevation", "Axial"))})
    X, Y, Z = np.meshgrid(vec["x"], vec["y"], vec["z"], indexing="ij")
    p = (1e5 * 10.0 ** (-(np.abs(X) * 2.0 + np.abs(Y) * 3.0 + np.abs(Z - 14.0) * 1.0) / 20.0)).astype(np.float32)      # 2 / 3 / 1 dB per mm
    p[0, 0, 0] = 0.0
    p[3, 3, 2] = 0.9 * p[3, 3, 2]       # a dip one step left of the peak on the x line is still above -6 dB
    na = np.full(p.shape, 7, dtype=np.int32)
    return SteeringMap.from_volumes(p, na, coords, reference=reference), p


def test_gain_envelope_and_constraints():
    sm, p = synthetic_map()
    assert sm.reference_index == (4, 3, 2)
    g = np.asarray(sm.dataset["steering_gain_db"].data)
    assert g[4, 3, 2] == 0.0 and g[0, 0, 0] == -np.inf and np.isneginf(steering_gain_db([0.0, 1.0], 1.0)[0])
    assert g[6, 3, 2] == pytest.approx(-4.0, abs=1e-4) and g[4, 3, 5] == pytest.approx(-6.0, abs=1e-4)
    assert np.array_equal(np.asarray(sm.dataset["n_active"].data), np.full(p.shape, 7)) and sm.dataset["focal_pressure"].attrs["units"] == "Pa"
    env = sm.envelope(-6.0)
    assert env.dtype == bool and np.array_equal(env, g >= -6.0) and env.sum() < env.size
    tcs = sm.to_target_constraints(-6.5)
    assert [(t.dim, t.units, t.min, t.max) for t in tcs] == [("x", "mm", -3.0, 3.0), ("y", "mm", -2.0, 2.0), ("z", "mm", 10.0, 20.0)]
    assert [t.name for t in tcs] == ["Lateral", "Elevation", "Axial"]
    proto = ol.Protocol(target_constraints=tcs)
    proto.check_target(ol.Point(position=(2.5, -1.0, 12.0), units="mm"))
    with pytest.raises(ValueError):
        proto.check_target(ol.Point(position=(3.5, 0.0, 12.0), units="mm"))


def test_the_run_is_contiguous_through_the_reference():
    sm, p = synthetic_map()
    p2 = p.copy(); p2[6, 3, 2] = 1.0          # a hole at x = +2 cuts the run although x = +3 is above -6.5 dB again
    sm2 = SteeringMap.from_volumes(p2, np.zeros(p.shape, np.int32), sm.dataset.coords)
    tx = sm2.to_target_constraints(-6.5)[0]
    assert (tx.min, tx.max) == (-3.0, 1.0)


def test_reference_point_and_its_refusal():
    sm, p = synthetic_map(reference=(2.2, -0.6, 15.1))        # nearest voxel: x = 2, y = -1, z = 16
    assert sm.reference_index == (6, 2, 3) and nearest_voxel((2.2, -0.6, 15.1), sm.dataset.coords) == (6, 2, 3)
    g = np.asarray(sm.dataset["steering_gain_db"].data)
    assert g[6, 2, 3] == 0.0 and g[4, 3, 2] == pytest.approx(9.0, abs=1e-4)
    with pytest.raises(ValueError, match="below"):
        sm.to_target_constraints(db=1.0)          # the reference voxel sits at 0 dB
    with pytest.raises(ValueError, match="outside"):
        synthetic_map(reference=(40.0, 0.0, 14.0))
    smp, _ = synthetic_map(reference=ol.Point(position=(2.2e-3, -0.6e-3, 15.1e-3), units="m"))
    assert smp.reference_index == (6, 2, 3)


# ---- refusals of calc_steering_map (before the device is touched) ------------------------------------------------------
def small_params():
    setup = ol.SimSetup(spacing=1.0, x_extent=(-3, 3), y_extent=(-3, 3), z_extent=(5, 11))
    return setup.setup_sim_scene(ol.seg.seg_methods.UniformWater())


def test_refusals():
    arr = ol.Transducer.gen_matrix_array(nx=2, ny=2, pitch=3, kerf=0.3, units="mm")
    params = small_params()
    with pytest.raises(NotImplementedError, match="MediumCompensated"):
        calc_steering_map(arr, params, apod_method=ol.apod_methods.MediumCompensated())
    arr.frequency = None
    with pytest.raises(ValueError, match="frequency"):
        calc_steering_map(arr, params)
    with pytest.raises(ValueError, match="frequency"):
        calc_steering_map(arr, params, freq=0.0)
    het = small_params()
    c = np.array(het["sound_speed"].data, dtype=np.float32)
    c[2, 2, 3:] = 2800.0
    het["sound_speed"] = ds.make_dataarray(c, coords=het.coords, dims=list(het.coords.keys()), name="sound_speed", attrs=dict(het["sound_speed"].attrs))
    with pytest.raises(NotImplementedError, match="heterogeneous"):
        calc_steering_map(arr, het, freq=F0)
