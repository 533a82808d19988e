"""Eikonal delays, host side (no GPU): the fp64 oracle (tests/eikonal_oracle.py) against the exact Snell travel times of a flat slab, in a
uniform medium and on an anisotropic grid; the oracle's delays fired through the full-wave oracle's wedge scene; the plug-in / Protocol JSON
round trips, params=None as Direct(c0), and every refusal raised before any device call (DESIGN.md section 2 "Eikonal").

Records (NumPy fp64; each assertion allows the record plus half again, the project's rule of section 2):
  scene A, largest error over the array relative to the centre element, in cycles at 500 kHz, against the Snell time:
    0.5 mm   (57 x 17 x 57, 84 sweeps)    Direct 0.139   StraightRay 0.0641   Eikonal 0.00965   (raw first-order eikonal time 0.115)
    0.375 mm (75 x 23 x 76, 113 sweeps)   Direct 0.132   StraightRay 0.0618   Eikonal 0.00820   (raw 0.0942)
  anisotropic spacing 0.4 / 0.5 / 0.3 mm, uniform 1500 m/s, largest |T - d / c| / (d / c) over seven directions at d = 2, 3.5, 5 mm:
    0.0836, 0.0796, 0.0693; at half the spacing 0.0779, 0.0601, 0.0491 (the first-order error around a point source: why the method
    uses only the difference of two solves)
  wedge scene (tests/fullwave_lockin_cases.py, 0.375 mm): forward steady focal amplitude with the Eikonal delays = 1.097 x that with
    Direct's and 0.970 x that with StraightRay's (TimeReversal: 1.162 x and 1.027 x); the focus is seven voxels deep, no ordering is asserted.
    The record of a ratio is its distance from 1 (+0.097, -0.030): the measured one stays within half of that of it"""
import json

import numpy as np
import pytest

import openlifu_amd as ol
from openlifu_amd import _native as nat
from openlifu_amd.bf import DelayMethod
from openlifu_amd.bf.delay_methods import Direct, Eikonal
from openlifu_amd.bf.delay_methods import eikonal as ek
import eikonal_cases as ec
import eikonal_oracle as eo
import fullwave_lockin_cases as lc
import medium_delay_oracle as mo

F0 = 500e3
SCENE_A = {0.5e-3: dict(n=(57, 17, 57), direct=0.139, ray=0.0641, eikonal=0.00965),
           0.375e-3: dict(n=(75, 23, 76), direct=0.132, ray=0.0618, eikonal=0.00820)}
ANISO = {1: (0.0836, 0.0796, 0.0693), 2: (0.0779, 0.0601, 0.0491)}
WEDGE = dict(over_direct=1.097, over_ray=0.970)


# ---- oracle: scene A --------------------------------------------------------------------------------------------------------------
def _scene_a_errors(h):
    sc = eo.scene_a(h)
    centre = len(sc["pos"]) // 2
    snell = np.array([eo.snell_time(np.hypot(p[0] - sc["focus"][0], p[1] - sc["focus"][1]), sc["layers"]) for p in sc["pos"]])
    r = eo.method(sc["pos"], sc["focus"], sc["c"].astype(np.float64), sc["origin"], sc["spacing"], sc["c_ref"])
    direct = np.linalg.norm(sc["pos"] - sc["focus"], axis=1) / sc["c_ref"]
    ray = mo.delays(sc["pos"], sc["focus"][None], sc["c"], sc["origin"], sc["spacing"], sc["c_ref"])[0]          # = max tau - tau
    err = {"direct": eo.relative_error_cycles(direct, snell, centre, F0), "ray": eo.relative_error_cycles(-ray, snell, centre, F0),
           "eikonal": eo.relative_error_cycles(r["tau"], snell, centre, F0), "raw": eo.relative_error_cycles(r["raw"], snell, centre, F0)}
    return sc, r, err


def test_oracle_scene_a_against_snell():
    errs = {}
    for h, rec in SCENE_A.items():
        sc, r, err = _scene_a_errors(h)
        print(f"scene A, h = {h * 1e3:g} mm, grid {sc['n']}, sweeps {r['sweeps']}: " + ", ".join(f"{k} {v:.4g}" for k, v in err.items()) + " cycles")
        assert sc["n"] == rec["n"] and len(sc["pos"]) == 9
        assert np.allclose(r["delays"], r["tau"].max() - r["tau"], rtol=0, atol=0)
        for key in ("direct", "ray", "eikonal"):
            assert err[key] <= 1.5 * rec[key], (h, key, err[key])
        assert err["eikonal"] <= 0.5 * err["ray"]
        assert err["raw"] > err["ray"]                 # the raw first-order time is worse than StraightRay: only the difference is used
        errs[h] = err["eikonal"]
    assert errs[0.375e-3] <= errs[0.5e-3]


# ---- oracle: uniform medium -------------------------------------------------------------------------------------------------------
def test_oracle_uniform_medium_is_direct():
    n, h, origin = (21, 17, 25), (0.5e-3, 0.5e-3, 0.5e-3), np.array([-5e-3, -4e-3, 0.0])
    pos = np.array([[-3.1e-3, 0.2e-3, 0.3e-3], [0.0, 0.0, 0.5e-3], [2.77e-3, -1.4e-3, 0.1e-3]])
    focus = np.array([0.2e-3, 0.1e-3, 9.3e-3])
    vol = np.full(n, 1500.0, dtype=np.float32).astype(np.float64)
    r = eo.method(pos, focus, vol, origin, h, 1500.0)
    assert np.array_equal(r["T_med"], r["T_ref"]) and np.isfinite(r["T_med"]).all()          # exactly 0 at every voxel
    assert np.array_equal(r["extra_path"], np.zeros(3)) and r["sweeps"][0] == r["sweeps"][1]
    tof = np.linalg.norm(pos - focus, axis=1) / 1500.0
    assert np.array_equal(r["delays"], tof.max() - tof)
    assert np.array_equal(r["delays"], mo.delays(pos, focus[None], None, origin, h, 1500.0)[0])


# ---- oracle: anisotropic spacing --------------------------------------------------------------------------------------------------
def _aniso_deviation(f):
    c, h0 = 1500.0, np.array([0.4e-3, 0.5e-3, 0.3e-3])
    n, origin = (30 * f + 1, 24 * f + 1, 40 * f + 1), np.array([-6e-3, -6e-3, 1e-3])
    src = origin + np.array([15.3, 11.6, 20.45]) * h0
    T, _ = eo.solve(n, origin, h0 / f, c, src)
    dirs = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, 1, 1], [-1, 0.5, -0.3], [0.2, -1, 0.7]], dtype=np.float64)
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    out = []
    for d in (2e-3, 3.5e-3, 5e-3):
        t = eo.sample(T, eo.trilinear_table(src + d * dirs, origin, h0 / f, n))
        out.append(float(np.abs(t - d / c).max() / (d / c)))
    return out


def test_oracle_anisotropic_spacing_converges_to_the_distance():
    coarse, fine = _aniso_deviation(1), _aniso_deviation(2)
    print("anisotropic spacing, |T - d / c| / (d / c) at d = 2, 3.5, 5 mm:", [f"{v:.4f}" for v in coarse], "halved:", [f"{v:.4f}" for v in fine])
    for got, rec in ((coarse, ANISO[1]), (fine, ANISO[2])):
        for g, r in zip(got, rec):
            assert g <= 1.5 * r, (got, rec)
    for a, b in zip(coarse, fine):
        assert b < a


def test_oracle_one_sweep_by_hand():
    """One sweep by hand on a 3 x 3 x 3 grid with three different spacings and equal neighbour times (a tie on every axis)"""
    h = (0.4e-3, 0.5e-3, 0.3e-3)
    T = np.full((3, 3, 3), np.inf)
    a = 2e-6
    T[0, 1, 1] = T[1, 0, 1] = T[1, 1, 0] = a
    frozen = np.isfinite(T)
    s = 1.0 / 1500.0
    out = eo.sweep(T, frozen, np.full(T.shape, s), h)
    w = [1.0 / v ** 2 for v in h]
    assert out[1, 1, 1] == a + np.sqrt(s * s / sum(w))            # all three axes: sum_a w_a x^2 = s^2
    assert np.array_equal(out[frozen], T[frozen])
    assert out[2, 1, 1] == np.inf                                   # nothing has arrived next to it yet
    T2 = np.full((3, 3, 3), np.inf)
    T2[0, 1, 1], T2[1, 0, 1] = a, a + 1e-3                         # the second neighbour is too late: one-axis update along x
    assert eo.sweep(T2, np.isfinite(T2), np.full(T.shape, s), h)[1, 1, 1] == a + s * h[0]


# ---- oracle: the wedge scene of the full-wave tests -------------------------------------------------------------------------------
def test_oracle_eikonal_delays_fired_through_the_wedge():
    h = 0.375e-3
    sc = lc.array_scene(h, "wedge")
    axis = lc.time_axis(sc)
    r = eo.method(sc["pos"], sc["focus"], sc["c"], (0.0, 0.0, 0.0), (h,) * 3, lc.C0)
    direct, ray = lc.direct_delays(sc), lc.straight_ray_delays(sc)
    assert np.abs(r["delays"] - direct).max() * F0 > 0.05           # the slab matters to the method
    a_ek, a_direct, a_ray = (lc.fire(sc, d, axis) for d in (r["delays"], direct, ray))
    print(f"forward steady focal amplitude: Eikonal / Direct = {a_ek / a_direct:.4f}, Eikonal / StraightRay = {a_ek / a_ray:.4f}")
    assert abs(a_ek / a_direct - WEDGE["over_direct"]) <= 0.5 * abs(WEDGE["over_direct"] - 1.0)
    assert abs(a_ek / a_ray - WEDGE["over_ray"]) <= 0.5 * abs(WEDGE["over_ray"] - 1.0)


# ---- plug-in, JSON ---------------------------------------------------------------------------------------------------------------
def test_plugin_lookup_and_protocol_json_round_trip():
    m = DelayMethod.from_dict({"class": "Eikonal", "c0": 1540, "init_radius": 2, "max_sweeps": 500})
    assert isinstance(m, Eikonal) and m.c0 == 1540.0 and m.init_radius == 2.0 and m.max_sweeps == 500
    assert m.to_dict() == {"c0": 1540.0, "init_radius": 2.0, "max_sweeps": 500, "class": "Eikonal"}
    assert DelayMethod.from_dict(m.to_dict()) == m
    assert DelayMethod.from_dict({"class": "Eikonal"}) == Eikonal() and Eikonal().init_radius == 3.0 and Eikonal().max_sweeps is None
    assert isinstance(ol.delay_methods.Eikonal(), DelayMethod) and "Eikonal" in ol.delay_methods.__all__
    proto = ol.Protocol(delay_method=Eikonal(c0=1520.0, init_radius=4.0))
    back = ol.Protocol.from_json(proto.to_json())
    assert type(back.delay_method) is Eikonal and back.delay_method == proto.delay_method
    assert json.loads(back.to_json(compact=True))["delay_method"] == {"c0": 1520.0, "init_radius": 4.0, "max_sweeps": None, "class": "Eikonal"}
    assert type(ol.Protocol().delay_method) is Direct        # the default stays Direct


@pytest.mark.parametrize("kw,exc", [(dict(c0=-1.0), ValueError), (dict(c0="fast"), TypeError), (dict(c0=True), TypeError), (dict(init_radius=0.5), ValueError),
                                    (dict(init_radius=float("nan")), ValueError), (dict(init_radius="3"), TypeError), (dict(max_sweeps=0), ValueError),
                                    (dict(max_sweeps=2.5), TypeError), (dict(max_sweeps=True), TypeError)])
def test_validation(kw, exc):
    with pytest.raises(exc):
        Eikonal(**kw)


# ---- params=None, fallbacks, refusals (a fake engine: any device call it does not expect fails the test) ----------------------------
class _Recorder:
    def __init__(self):
        self.calls = []

    def beamform(self, arr, targets, c, transform=None, apod=None):
        self.calls.append(("beamform", c, transform))
        n = len(targets) if isinstance(targets, (list, tuple)) else 1
        return np.zeros((n, 4)), np.ones((n, 4))

    def eikonal(self, *a, **k):
        self.calls.append(("eikonal",) + a)
        raise AssertionError("device call")


@pytest.fixture
def rec(monkeypatch):
    r = _Recorder()
    monkeypatch.setattr(ek, "get_engine", lambda: r)
    return r


def test_params_none_is_direct_c0(rec):
    arr = ol.Transducer.gen_matrix_array(2, 2, 2.0, 0.5)
    M = np.eye(4)
    d = Eikonal(c0=1490.0).calc_delays(arr, ol.Point(position=(0, 0, 30)), transform=M)
    assert d.shape == (4,) and rec.calls == [("beamform", 1490.0, M)]
    assert Eikonal(c0=1490.0).calc_delays(arr, [ol.Point(position=(0, 0, 30))] * 3).shape == (3, 4)
    delays, info = Eikonal().solve(arr, ol.Point(position=(0, 0, 30)))
    assert delays.shape == (1, 4) and info == {"extra_path_m": [], "travel_time_s": [], "sweeps": []}


def test_a_medium_that_is_c_ref_everywhere_runs_no_solve(rec):
    arr = ol.Transducer.gen_matrix_array(2, 2, 2.0, 0.5)
    p = ec.Params((9, 8, 12), (-4e-3, -3.5e-3, 0.0), (1e-3, 1e-3, 1e-3), 1500.0, uniform_value=1500.0)     # a constant volume nobody has touched
    d = Eikonal().calc_delays(arr, ol.Point(position=(0, 0, 6)), p)
    assert d.shape == (4,) and rec.calls == [("beamform", 1500.0, None)]          # kernel 1 at c_ref, nothing else


@pytest.mark.parametrize("case", ["shape", "zero", "nan", "c_ref_zero", "target_outside", "target_nan", "element_outside", "transform_shape",
                                  "element_outside_by_transform"])
def test_refusals_before_any_device_call(rec, case):
    arr = ol.Transducer.gen_matrix_array(2, 2, 2.0, 0.5)       # elements at x, y = +-1 mm, z = 0
    vol, ref, target, M = np.full((9, 8, 12), 1500.0, dtype=np.float32), 1500.0, ol.Point(position=(0, 0, 6)), None
    match = "Eikonal"
    if case == "shape":
        vol, match = np.full((9, 8, 11), 1500.0, dtype=np.float32), "does not match the grid"
    elif case in ("zero", "nan"):
        vol[1, 1, 1], match = {"zero": 0.0, "nan": np.nan}[case], "sound speed"
    elif case == "c_ref_zero":
        ref, match = 0.0, "reference sound speed"
    elif case == "target_outside":
        target, match = ol.Point(position=(0, 0, 11.5)), "Eikonal: target 0"
    elif case == "target_nan":
        target, match = np.array([[0.0, np.nan, 6e-3]]), "Eikonal: target 0"
    elif case == "element_outside":
        arr, match = ol.Transducer.gen_matrix_array(2, 2, 9.0, 0.5), "Eikonal: element 0"          # x = +-4.5 mm: half a voxel outside
    elif case == "transform_shape":
        M, match = np.eye(3), "4 x 4"
    elif case == "element_outside_by_transform":
        M = np.eye(4); M[2, 3] = -1e-3
        match = "Eikonal: element 0"
    p = ec.Params(vol, (-4e-3, -3.5e-3, 0.0), (1e-3, 1e-3, 1e-3), ref, n=(9, 8, 12))
    if case not in ("shape", "zero", "nan", "c_ref_zero"):
        vol[4, 4, 3] = 2800.0
    with pytest.raises(ValueError, match=match):
        Eikonal().calc_delays(arr, target, p, transform=M)
    if M is None:
        with pytest.raises(ValueError, match=match):
            ol.Protocol(delay_method=Eikonal()).beamform(arr, target, p)
    assert rec.calls == []


def test_the_solves_get_the_medium_then_the_reference(monkeypatch):
    """What reaches the engine: per focus the params volume, then c_ref, from the target, with the elements' trilinear table"""
    seen = []

    class Eng:
        def eikonal(self, origin, spacing, n, c, src, points, init_radius, max_sweeps, volume=False):
            seen.append((np.ndim(c), np.array(src), init_radius, max_sweeps, volume))
            row, vox, wt = points
            assert len(row) == 5 and row[-1] == len(vox) == len(wt)
            t = np.full(4, 7e-6) if np.ndim(c) else np.full(4, 6e-6)
            return t, 11 if np.ndim(c) else 10, (np.zeros(n, dtype=np.float32) if volume else None)

    monkeypatch.setattr(ek, "get_engine", lambda: Eng())
    arr = ol.Transducer.gen_matrix_array(2, 2, 2.0, 0.5)
    vol = np.full((9, 8, 12), 1500.0, dtype=np.float32); vol[:, :, 3] = 2800.0
    p = ec.Params(vol, (-4e-3, -3.5e-3, 0.0), (1e-3, 1e-3, 1e-3), 1500.0)
    foci = [ol.Point(position=(0, 0, 6)), ol.Point(position=(0.5, 0, 7))]
    delays, info = Eikonal(init_radius=2, max_sweeps=77).solve(arr, foci, p, return_volumes=True)
    assert [s[0] for s in seen] == [3, 0, 3, 0] and all(s[2:] == (2.0, 77, True) for s in seen)
    assert np.allclose(seen[2][1], [0.5e-3, 0, 7e-3]) and delays.shape == (2, 4)
    assert info["sweeps"] == [(11, 10), (11, 10)] and len(info["volumes"]) == 2
    assert np.allclose(info["extra_path_m"][0], 1500.0 * 1e-6)
    pos = arr.element_table()[0]
    tau = np.linalg.norm(pos - [0, 0, 6e-3], axis=1) / 1500.0 + 1e-6
    assert np.allclose(info["travel_time_s"][0], tau, rtol=1e-14) and np.allclose(delays[0], tau.max() - tau, rtol=0, atol=1e-20)


def test_native_error_without_a_gpu():
    if nat.device_count() > 0:
        pytest.skip("GPU present")
    arr = ol.Transducer.gen_matrix_array(2, 2, 2.0, 0.5)
    vol = np.full((9, 8, 12), 1500.0, dtype=np.float32); vol[:, :, 3] = 2800.0
    p = ec.Params(vol, (-4e-3, -3.5e-3, 0.0), (1e-3, 1e-3, 1e-3), 1500.0)
    with pytest.raises(nat.NativeError):
        Eikonal().calc_delays(arr, ol.Point(position=(0, 0, 6)), p)
    with pytest.raises(nat.NativeError):
        Eikonal().calc_delays(arr, ol.Point(position=(0, 0, 6)))


def test_symbols_and_error_code():
    for s in ("olx_eikonal_solve", "olx_eikonal_sample", "olx_eikonal_fetch"):
        assert s in nat.SYMBOLS
    assert nat.OLX_ENOCONV == -6 and issubclass(nat.ConvergenceError, nat.NativeError)
