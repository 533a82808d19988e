"""StraightRay delays, host side (no GPU): the fp64 oracle (tests/medium_delay_oracle.py) against known answers and against the phase of the
sampled straight-ray field model of oracle/field_oracle.c, the plug-in / Protocol JSON round trips, params=None as Direct(c0), and every
refusal raised before any device call (DESIGN.md section 2 "StraightRay")."""
import json
from types import SimpleNamespace

import numpy as np
import pytest

import openlifu_amd as ol
from openlifu_amd.bf import DelayMethod
from openlifu_amd.bf.delay_methods import Direct, StraightRay
from openlifu_amd.bf.delay_methods import straightray as sr
from oracle import c_oracle as co
import medium_delay_oracle as mo

C = 1500.0


def _grid(n=(9, 8, 12), h=1e-3, z0=5e-3):
    origin = (-(n[0] - 1) / 2 * h, -(n[1] - 1) / 2 * h, z0)
    axes = [origin[a] + np.arange(n[a]) * h for a in range(3)]
    return origin, (h, h, h), axes


# ---- oracle -----------------------------------------------------------------------------------------------------------------------
def test_oracle_uniform_medium_is_direct():
    origin, spacing, (xs, ys, zs) = _grid()
    pos = np.array([[0.0, 0.0, 0.0], [2e-3, -1e-3, 0.0], [-3e-3, 2e-3, 1e-3]])
    foci = [[0.0, 0.0, 12e-3], [1.5e-3, 0.7e-3, 14.3e-3]]
    vol = np.full((9, 8, 12), C, dtype=np.float32)
    for f in foci:
        assert np.array_equal(mo.extra_path(mo.sigma(vol, C), origin, spacing, pos, np.array(f)), np.zeros(3))
    tof = np.linalg.norm(np.asarray(foci)[:, None, :] - pos[None], axis=2) / C
    assert np.allclose(mo.delays(pos, foci, vol, origin, spacing, C), tof.max(axis=1, keepdims=True) - tof, rtol=0, atol=1e-18)
    assert np.array_equal(mo.delays(pos, foci, vol, origin, spacing, C), mo.delays(pos, foci, None, origin, spacing, C))


@pytest.mark.parametrize("m", [1, 3])
def test_oracle_laterally_uniform_slab(m):
    """An m-plane slab wholly between element and focus: E = m hz d / |dz| sigma."""
    origin, spacing, (xs, ys, zs) = _grid()
    vol = np.full((9, 8, 12), C, dtype=np.float32)
    vol[:, :, 3:3 + m] = 2500.0
    sig = float(mo.sigma(np.float32(2500.0), C))
    pos = np.array([[0.0, 0.0, 0.0], [3e-3, -2e-3, 1e-3], [-20e-3, 9e-3, 0.0]])      # (the last one far outside the lateral extent)
    focus = np.array([0.4e-3, -0.3e-3, 13.6e-3])
    d = np.linalg.norm(focus - pos, axis=1)
    E = mo.extra_path(mo.sigma(vol, C), origin, spacing, pos, focus)
    assert np.allclose(E, m * 1e-3 * d / np.abs(focus[2] - pos[:, 2]) * sig, rtol=1e-13, atol=0)


def test_oracle_matches_the_sampled_field_model_at_voxels():
    """At grid voxels E is the E of olo_field_grid_hetero: one element, a low-contrast medium, k E recovered from the phase of the
    heterogeneous field over the homogeneous one (no attenuation)."""
    origin, spacing, (xs, ys, zs) = _grid(n=(9, 8, 14))
    rng = np.random.default_rng(5)
    vol = (C + rng.uniform(-25, 25, (9, 8, 14))).astype(np.float32)
    vol[:, :, :2] = C
    sig = mo.sigma(vol, C)
    for pos in ([[0.3e-3, -0.2e-3, 0.0]], [[-1.2e-3, 0.9e-3, 8.2e-3]]):       # below the grid, inside it
        pos = np.asarray(pos)
        f0 = 400e3
        het = co.field_on_grid_hetero(xs, ys, zs, sig, np.zeros_like(sig), pos, [1e-6], [0.0], [1.0], f0, C, 1.0, dmin=0.5e-3)
        hom = co.field_on_grid_hetero(xs, ys, zs, np.zeros_like(sig), np.zeros_like(sig), pos, [1e-6], [0.0], [1.0], f0, C, 1.0, dmin=0.5e-3)
        k = 2 * np.pi * f0 / C
        worst = 0.0
        for i, j, kv in [(0, 0, 13), (4, 3, 10), (8, 7, 2), (2, 5, 7), (6, 1, 13), (4, 4, 11)]:
            E = mo.extra_path(sig, origin, spacing, pos, np.array([xs[i], ys[j], zs[kv]]))[0]
            got = np.angle(het[i, j, kv] / hom[i, j, kv])
            worst = max(worst, abs(got - k * E))
            assert abs(k * E) < 3.0
        assert worst <= 1e-9, worst


# ---- plug-in, JSON ---------------------------------------------------------------------------------------------------------------
def test_plugin_lookup_and_protocol_json_round_trip():
    m = DelayMethod.from_dict({"class": "StraightRay", "c0": 1540})
    assert isinstance(m, StraightRay) and m.c0 == 1540.0
    assert m.to_dict() == {"c0": 1540.0, "class": "StraightRay"}
    assert DelayMethod.from_dict(m.to_dict()) == m
    assert isinstance(ol.delay_methods.StraightRay(), DelayMethod)
    with pytest.raises(ValueError):
        StraightRay(c0=-1.0)
    with pytest.raises(TypeError):
        StraightRay(c0="fast")
    proto = ol.Protocol(delay_method=StraightRay(c0=1520.0))
    back = ol.Protocol.from_json(proto.to_json())
    assert type(back.delay_method) is StraightRay and back.delay_method.c0 == 1520.0
    assert json.loads(back.to_json(compact=True))["delay_method"] == {"c0": 1520.0, "class": "StraightRay"}
    assert type(ol.Protocol().delay_method) is Direct        # the default stays Direct


# ---- params=None, refusals (a fake engine: any device call fails the test) ---------------------------------------------------------
class _Recorder:
    def __init__(self):
        self.calls = []

    def beamform(self, arr, targets, c, transform=None, apod=None):
        self.calls.append(("beamform", c, transform))
        n = len(targets) if isinstance(targets, (list, tuple)) else 1
        return np.zeros((n, 4)), np.ones((n, 4))

    def beamform_medium(self, *a, **k):
        self.calls.append(("beamform_medium",) + a)
        raise AssertionError("device call")


def test_params_none_is_direct_c0(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(sr, "get_engine", lambda: rec)
    arr = ol.Transducer.gen_matrix_array(2, 2, 2.0, 0.5)
    M = np.eye(4)
    d = StraightRay(c0=1490.0).calc_delays(arr, ol.Point(position=(0, 0, 30)), transform=M)
    assert d.shape == (4,) and rec.calls == [("beamform", 1490.0, M)]
    assert StraightRay(c0=1490.0).calc_delays(arr, [ol.Point(position=(0, 0, 30))] * 3).shape == (3, 4)


class _P:
    """The part of a params Dataset StraightRay reads: coords and params["sound_speed"] (data, attrs["ref_value"])."""

    def __init__(self, vol, ref=C, n=(6, 5, 4)):
        setup = ol.SimSetup(spacing=1.0, x_extent=(0, n[0] - 1), y_extent=(0, n[1] - 1), z_extent=(10, 10 + n[2] - 1))
        self.coords = setup.get_coords()
        self._ss = SimpleNamespace(data=vol, attrs={"ref_value": ref})

    def __getitem__(self, key):
        return self._ss


@pytest.mark.parametrize("case", ["shape", "zero", "negative", "nan", "inf", "c_ref_zero", "c_ref_negative", "c_ref_nan"])
def test_refusals_before_any_device_call(monkeypatch, case):
    rec = _Recorder()
    monkeypatch.setattr(sr, "get_engine", lambda: rec)
    vol = np.full((6, 5, 4), C, dtype=np.float32)
    ref = C
    if case == "shape":
        vol = np.full((6, 5, 5), C, dtype=np.float32)
    elif case in ("zero", "negative", "nan", "inf"):
        vol[2, 3, 1] = {"zero": 0.0, "negative": -1500.0, "nan": np.nan, "inf": np.inf}[case]
    else:
        ref = {"c_ref_zero": 0.0, "c_ref_negative": -1.0, "c_ref_nan": float("nan")}[case]
    arr = ol.Transducer.gen_matrix_array(2, 2, 2.0, 0.5)
    with pytest.raises(ValueError, match="StraightRay"):
        StraightRay().calc_delays(arr, ol.Point(position=(0, 0, 12)), _P(vol, ref))
    with pytest.raises(ValueError, match="StraightRay"):
        ol.Protocol(delay_method=StraightRay()).beamform_foci(arr, [ol.Point(position=(0, 0, 12))], _P(vol, ref))
    assert rec.calls == []


def test_uniform_declared_medium_uploads_no_volume():
    """A constant volume nobody touched (uniform_value) is not scanned: c_ref everywhere uploads nothing, another constant a full volume."""
    p = _P(None)
    p._ss = SimpleNamespace(uniform_value=C, attrs={"ref_value": C})
    c_ref, vol, origin, spacing, n = StraightRay.medium(p)
    assert c_ref == C and vol is None and tuple(n) == (6, 5, 4) and np.allclose(spacing, 1e-3)
    p._ss = SimpleNamespace(uniform_value=1540.0, attrs={"ref_value": C})
    _, vol, _, _, _ = StraightRay.medium(p)
    assert vol.shape == (6, 5, 4) and vol.dtype == np.float32 and (vol == 1540.0).all()
