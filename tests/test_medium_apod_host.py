"""MediumCompensated apodization, host side (no GPU): the fp64 oracle (tests/medium_apod_oracle.py) against known answers, the plug-in /
Protocol JSON round trips, params=None as the base method, and every refusal raised before any device call (DESIGN.md section 2
"MediumCompensated")."""
import json
from types import SimpleNamespace

import numpy as np
import pytest

import openlifu_amd as ol
from openlifu_amd.bf import ApodizationMethod
from openlifu_amd.bf.apod_methods import MaxAngle, MediumCompensated, PiecewiseLinear, Uniform
from openlifu_amd.bf.apod_methods import mediumcompensated as mc
from openlifu_amd.bf.delay_methods import Direct, StraightRay
from openlifu_amd.sim.field import _np_per_m
import medium_apod_oracle as ao

F0 = 400e3


def _grid(n=(9, 8, 12), h=1e-3, z0=5e-3):
    origin = (-(n[0] - 1) / 2 * h, -(n[1] - 1) / 2 * h, z0)
    axes = [origin[a] + np.arange(n[a]) * h for a in range(3)]
    return origin, (h, h, h), axes


# ---- oracle -----------------------------------------------------------------------------------------------------------------------
def test_oracle_unit_conversion_is_the_field_models():
    for alpha in (0.0, 0.3, 6.0):
        assert ao.np_per_m(np.float32(alpha), F0) == pytest.approx(_np_per_m(np.float32(alpha), F0), rel=1e-15, abs=0)


@pytest.mark.parametrize("m", [1, 3])
def test_oracle_laterally_uniform_slab(m):
    """m lossy planes (T = m hz) with zero planes on both sides, wholly between element and focus: A = a T d / |dz| exactly."""
    origin, spacing, (xs, ys, zs) = _grid()
    vol = np.zeros((9, 8, 12), dtype=np.float32)
    vol[:, :, 3:3 + m] = 6.0
    a = float(ao.np_per_m(np.float32(6.0), F0))
    pos = np.array([[0.0, 0.0, 0.0], [3e-3, -2e-3, 1e-3], [-20e-3, 9e-3, 0.0]])      # (the last one far outside the lateral extent)
    for focus in (np.array([xs[5], ys[2], zs[10]]), np.array([0.4e-3, -0.3e-3, 13.6e-3])):      # on a voxel, off the voxels
        d = np.linalg.norm(focus - pos, axis=1)
        A, d_o = ao.ray_sums(ao.np_per_m(vol, F0), origin, spacing, pos, focus)
        ref = a * m * 1e-3 * d / np.abs(focus[2] - pos[:, 2])
        assert np.abs(A / ref - 1).max() <= 1e-12 and np.array_equal(d_o, d)
        _, h, _ = ao.arrival(pos, focus, vol, origin, spacing, F0)
        assert np.allclose(h[0], np.exp(-ref), rtol=1e-12, atol=0)


def test_oracle_no_attenuation_and_level_rays():
    origin, spacing, _ = _grid()
    pos = np.array([[0.0, 0.0, 0.0], [2e-3, 1e-3, 9e-3]])
    b = np.array([[1.0, 0.5]])
    for vol in (None, np.zeros((9, 8, 12), dtype=np.float32)):
        for mode in ("equalize", "matched"):
            assert np.array_equal(ao.apodization(pos, [[0, 0, 14e-3]], b, vol, origin, spacing, F0, mode=mode), b)
    vol = np.full((9, 8, 12), 3.0, dtype=np.float32)
    A, _, _ = ao.arrival(pos, [[0.5e-3, 0, 9e-3]], vol, origin, spacing, F0)          # the second element at the focus' height: dz == 0
    assert A[0, 1] == 0.0 and A[0, 0] > 0


def test_oracle_modes():
    """"matched" maximises sum apod h / sqrt(sum apod^2) (Cauchy-Schwarz); "equalize" makes apod h constant over the active set; inactive
    elements stay off, one active element keeps its base weight, apod <= b."""
    rng = np.random.default_rng(11)
    h = rng.uniform(0.2, 1.0, (1, 40))
    ones = np.ones((1, 40))
    gain = lambda w: (w * h[0]).sum() / np.sqrt((w * w).sum())
    matched = ao.compensate(ones, h, "matched")[0]
    best = gain(matched)
    assert matched.max() == 1.0
    for _ in range(1000):
        assert gain(rng.uniform(0.0, 1.0, 40)) <= best
    assert gain(ones[0]) < best
    b = rng.uniform(0.1, 1.0, (1, 40)); b[0, ::3] = 0.0
    for mode in ("equalize", "matched"):
        w = ao.compensate(b, h, mode)
        assert np.array_equal(w == 0, b == 0) and (w <= b).all() and (w >= 0).all()
    act = b[0] > 0
    eq = ao.compensate((b > 0).astype(float), h, "equalize")[0]
    arrive = (eq * h[0])[act]
    assert np.abs(arrive / arrive[0] - 1).max() <= 1e-14 and eq.max() == 1.0
    one = np.zeros((1, 40)); one[0, 7] = 0.6
    for mode in ("equalize", "matched"):
        assert np.array_equal(ao.compensate(one, h, mode), one)
        assert np.array_equal(ao.compensate(np.zeros((1, 40)), h, mode), np.zeros((1, 40)))
    with pytest.raises(ValueError):
        ao.compensate(b, h, "loud")


# ---- plug-in, JSON ---------------------------------------------------------------------------------------------------------------
def test_dataclass_validation():
    m = MediumCompensated()
    assert type(m.base) is Uniform and m.mode == "equalize" and m.spreading is False and m.frequency is None
    assert MediumCompensated(base={"class": "MaxAngle", "max_angle": 40.0}).base == MaxAngle(max_angle=40.0)
    assert MediumCompensated(base=PiecewiseLinear(80.0, 30.0)).kernel_args() == PiecewiseLinear(80.0, 30.0).kernel_args()
    assert MediumCompensated(frequency=500000).frequency == 500e3
    for bad in (MediumCompensated(), Direct(), "Uniform", None, 3):
        with pytest.raises(TypeError, match="Base"):
            MediumCompensated(base=bad)
    with pytest.raises(ValueError, match="Mode"):
        MediumCompensated(mode="loud")
    with pytest.raises(TypeError, match="Spreading"):
        MediumCompensated(spreading="yes")
    with pytest.raises(TypeError, match="Frequency"):
        MediumCompensated(frequency="high")
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="Frequency"):
            MediumCompensated(frequency=bad)


def test_plugin_lookup_and_protocol_json_round_trip():
    m = ApodizationMethod.from_dict({"class": "MediumCompensated", "base": {"class": "MaxAngle", "max_angle": 50}, "mode": "matched",
                                     "spreading": True, "frequency": 4e5})
    assert isinstance(m, MediumCompensated) and m.base == MaxAngle(max_angle=50) and m.mode == "matched" and m.spreading and m.frequency == 4e5
    assert m.to_dict() == {"base": {"max_angle": 50, "units": "deg", "class": "MaxAngle"}, "mode": "matched", "spreading": True,
                           "frequency": 4e5, "class": "MediumCompensated"}
    assert ApodizationMethod.from_dict(m.to_dict()) == m
    assert ApodizationMethod.from_dict(json.loads(json.dumps(m.to_dict()))) == m
    assert isinstance(ol.apod_methods.MediumCompensated(), ApodizationMethod)
    assert type(ApodizationMethod.from_dict({"class": "MediumCompensated"}).base) is Uniform
    d = ol.Protocol().to_dict()
    d["apod_method"] = {"class": "MediumCompensated"}
    proto = ol.Protocol.from_dict(d)
    assert proto.apod_method == MediumCompensated() and proto._fused()
    proto = ol.Protocol(apod_method=MediumCompensated(base=PiecewiseLinear(70.0, 20.0), mode="matched"), delay_method=StraightRay())
    back = ol.Protocol.from_json(proto.to_json())
    assert back.apod_method == proto.apod_method and type(back.apod_method.base) is PiecewiseLinear
    assert json.loads(back.to_json(compact=True))["apod_method"]["base"]["class"] == "PiecewiseLinear"
    assert type(ol.Protocol().apod_method) is Uniform        # the default stays Uniform


# ---- params=None, refusals (a fake engine: any device call fails the test) ---------------------------------------------------------
class _Recorder:
    def __init__(self):
        self.calls = []

    def beamform(self, arr, targets, c, transform=None, apod=None):
        self.calls.append(("beamform", c, transform, apod))
        n = len(targets) if isinstance(targets, (list, tuple)) else 1
        return np.zeros((n, 4)), np.ones((n, 4))

    def beamform_compensated(self, *a, **k):
        self.calls.append(("beamform_compensated",) + a)
        raise AssertionError("device call")

    def beamform_medium(self, *a, **k):
        self.calls.append(("beamform_medium",) + a)
        raise AssertionError("device call")


def test_params_none_is_the_base_method(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(mc, "get_engine", lambda: rec)
    arr = ol.Transducer.gen_matrix_array(2, 2, 2.0, 0.5)
    M = np.eye(4)
    base = MaxAngle(max_angle=35.0)
    a = MediumCompensated(base=base, mode="matched", spreading=True).calc_apodization(arr, ol.Point(position=(0, 0, 30)), transform=M)
    assert a.shape == (4,) and rec.calls == [("beamform", 1.0, M, base.kernel_args())]
    assert MediumCompensated().calc_apodization(arr, [ol.Point(position=(0, 0, 30))] * 3).shape == (3, 4)
    rec.calls.clear()
    ol.Protocol(apod_method=MediumCompensated(base=base), delay_method=Direct(c0=1490.0)).beamform_foci(arr, [ol.Point(position=(0, 0, 30))], None)
    assert rec.calls == [("beamform", 1490.0, None, base.kernel_args())]


class _P:
    """The part of a params Dataset the methods read: coords, params["attenuation"] (data) and params["sound_speed"] (data, ref_value)."""

    def __init__(self, vol, n=(6, 5, 4)):
        setup = ol.SimSetup(spacing=1.0, x_extent=(0, n[0] - 1), y_extent=(0, n[1] - 1), z_extent=(10, 10 + n[2] - 1))
        self.coords = setup.get_coords()
        self.vols = {"attenuation": SimpleNamespace(data=vol, attrs={"ref_value": 0.0}),
                     "sound_speed": SimpleNamespace(uniform_value=1500.0, attrs={"ref_value": 1500.0})}

    def __getitem__(self, key):
        return self.vols[key]


@pytest.mark.parametrize("delay_method", [Direct(), StraightRay()])
@pytest.mark.parametrize("case", ["shape", "negative", "nan", "inf", "no_frequency"])
def test_refusals_before_any_device_call(monkeypatch, case, delay_method):
    rec = _Recorder()
    monkeypatch.setattr(mc, "get_engine", lambda: rec)
    vol = np.zeros((6, 5, 4), dtype=np.float32)
    freq = F0
    if case == "shape":
        vol = np.zeros((6, 5, 5), dtype=np.float32)
    elif case == "no_frequency":
        freq = None
    else:
        vol[2, 3, 1] = {"negative": -0.5, "nan": np.nan, "inf": np.inf}[case]
    arr = ol.Transducer.gen_matrix_array(2, 2, 2.0, 0.5)
    with pytest.raises(ValueError, match="MediumCompensated"):
        MediumCompensated(frequency=freq).calc_apodization(arr, ol.Point(position=(0, 0, 12)), _P(vol))
    with pytest.raises(ValueError, match="MediumCompensated"):
        MediumCompensated(frequency=freq).solve(arr, [ol.Point(position=(0, 0, 12))], _P(vol), delay_method=delay_method)
    if case != "no_frequency":       # (a Protocol supplies its pulse's frequency)
        with pytest.raises(ValueError, match="MediumCompensated"):
            ol.Protocol(apod_method=MediumCompensated(), delay_method=delay_method).beamform_foci(arr, [ol.Point(position=(0, 0, 12))], _P(vol))
    assert rec.calls == []


def test_native_mode_is_refused_on_the_host():
    from openlifu_amd import _native as nat
    ctx = nat.Context.__new__(nat.Context)          # no library, no device: the check comes first
    with pytest.raises(ValueError, match="mode"):
        nat.Context.bf_solve_compensated(ctx, [[0, 0, 1e-2]], 1500.0, mode="loud")


def test_protocol_passes_its_pulse_frequency_and_the_delay_medium(monkeypatch):
    seen = {}

    class _Engine:
        def beamform_compensated(self, arr, targets, c, att, origin, spacing, n, freq, transform=None, apod=None, mode=None, spreading=None,
                                 sound_speed=False):
            seen.update(c=c, att=att, freq=freq, mode=mode, spreading=spreading, sound_speed=sound_speed, apod=apod)
            return np.zeros((1, 4)), np.ones((1, 4))

    monkeypatch.setattr(mc, "get_engine", lambda: _Engine())
    arr = ol.Transducer.gen_matrix_array(2, 2, 2.0, 0.5)
    vol = np.zeros((6, 5, 4), dtype=np.float32); vol[:, :, 1] = 2.0
    proto = ol.Protocol(pulse=ol.Pulse(frequency=650e3), apod_method=MediumCompensated(mode="matched", spreading=True))
    d, a, resident = proto.beamform_foci(arr, [ol.Point(position=(0, 0, 12))], _P(vol))
    assert resident and seen["freq"] == 650e3 and seen["c"] == 1500.0 and seen["sound_speed"] is False
    assert seen["mode"] == "matched" and seen["spreading"] is True and np.array_equal(seen["att"], vol)
    proto.apod_method.frequency = 300e3                       # the method's own frequency wins
    proto.delay_method = StraightRay()
    proto.beamform_foci(arr, [ol.Point(position=(0, 0, 12))], _P(vol))
    assert seen["freq"] == 300e3 and seen["sound_speed"] is None      # (c_ref everywhere: StraightRay.medium's None)


def test_uniform_declared_attenuation_uploads_no_volume():
    p = _P(None)
    p.vols["attenuation"] = SimpleNamespace(uniform_value=0.0, attrs={"ref_value": 0.0})
    vol, origin, spacing, n = MediumCompensated.medium(p)
    assert vol is None and tuple(n) == (6, 5, 4) and np.allclose(spacing, 1e-3)
    p.vols["attenuation"] = SimpleNamespace(uniform_value=0.3, attrs={"ref_value": 0.0})
    vol, _, _, _ = MediumCompensated.medium(p)
    assert vol.shape == (6, 5, 4) and vol.dtype == np.float32 and (vol == np.float32(0.3)).all()
