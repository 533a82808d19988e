"""Steering map through a medium on the host: the fp64 oracle (tests/steering_medium_oracle.py) against the oracles of kernels 1a / 1m / 4 and
closed forms of the definition (DESIGN.md section 2 "Steering map through a medium"), and the argument handling of
``calc_steering_map(medium_model=...)`` with the engine stubbed -- nothing here touches the device."""
import numpy as np
import pytest

import openlifu_amd as ol
from openlifu_amd.plan import calc_steering_map
from openlifu_amd.plan import steering as steering_mod
from openlifu_amd.util import dataset as ds
import medium_apod_oracle as mao
import medium_delay_oracle as mdo
import steering_medium_oracle as smo
import steering_oracle as so

F0, C, P0 = 400e3, 1500.0, 1e5
LAM = C / F0


def scene():
    """4 x 4 elements near z = 0 (z jittered off the planes, normals tilted), a 12 x 10 x 14 grid at 1 mm through the element plane, and a phantom
    whose slab (planes 6 .. 10) varies with x and y in thickness and value; a second region on planes 0 .. 1 below the array."""
    rng = np.random.default_rng(3)
    gx, gy = np.meshgrid((np.arange(4) - 1.5) * 3e-3, (np.arange(4) - 1.5) * 3e-3, indexing="ij")
    pos = np.stack([gx.ravel(), gy.ravel(), rng.uniform(-0.4e-3, 0.4e-3, 16)], axis=1) + rng.uniform(-0.2e-3, 0.2e-3, (16, 3)) * [1, 1, 0]
    nrm = np.tile([0.0, 0.0, 1.0], (16, 1)) + rng.uniform(-0.1, 0.1, (16, 3))
    area = np.full(16, 2.7e-3 * 2.7e-3) * rng.uniform(0.8, 1.2, 16)
    n, spacing, origin = (12, 10, 14), (1e-3, 1e-3, 1e-3), (-5.5e-3, -4.5e-3, -2e-3)
    I, J, K = np.meshgrid(*(np.arange(m) for m in n), indexing="ij")
    slab = (K >= 6 + (I + J) % 2) & (K <= 10 - (I // 4) % 2)
    below = K <= 1
    ss = np.full(n, C, dtype=np.float32)
    ss[slab] = (2800.0 * (1 + 0.05 * np.sin(0.7 * I + 0.4 * J)))[slab]
    ss[below] = (1700.0 + 10.0 * I)[below]
    att = np.zeros(n, dtype=np.float32)
    att[slab] = (8.0 * (1 + 0.2 * np.cos(0.5 * I - 0.3 * J)))[slab]
    att[below] = (2.0 + 0.1 * J)[below]
    return dict(pos=pos, nrm=nrm, area=area, n=n, spacing=spacing, origin=origin, ss=ss, att=att)


def test_ray_sums_and_amplitudes_are_kernel_1a_and_1m_with_the_voxel_as_focus():
    s = scene()
    rng = np.random.default_rng(21)
    vox = np.stack([rng.integers(0, m, 20) for m in s["n"]], axis=1)
    A, E = smo.medium_sums(s["origin"], s["spacing"], s["n"], s["pos"], F0, C, s["ss"], s["att"], voxels=vox)
    sig = mdo.sigma(s["ss"], C)
    nrm = s["nrm"] / np.linalg.norm(s["nrm"], axis=1)[:, None]
    for q, (i, j, k) in enumerate(vox):
        r = np.array([s["origin"][a] + (i, j, k)[a] * s["spacing"][a] for a in range(3)])
        for spreading in (False, True):
            A_ref, h_ref, d_ref = mao.arrival(s["pos"], r, s["att"], s["origin"], s["spacing"], F0, area=s["area"] if spreading else None)
            assert np.abs(A[q] - A_ref[0]).max() <= 1e-12 * np.abs(A_ref).max(), (q, spreading)
            b = smo.base_apodization((r - s["pos"])[None, :, :], nrm, ("maxangle", 35.0, 0.0))
            assert 0 < (b > 0).sum() < b.size or q > 0
            dc = np.maximum(d_ref, 0.5e-3)
            h = np.exp(-A[q])[None, :] * (s["area"][None, :] / dc if spreading else 1.0)
            for mode in ("equalize", "matched"):
                ref = mao.compensate(b, h_ref, mode)
                got = smo.compensated(b, h, mode)
                assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max(), (q, spreading, mode)
        E_ref = mdo.extra_path(sig, s["origin"], s["spacing"], s["pos"], r)
        assert np.abs(E[q] - E_ref).max() <= 1e-12 * np.abs(E_ref).max(), q
    assert np.abs(A).max() > 0.1 and np.abs(E).max() > 1e-3          # the phantom is on the rays


@pytest.mark.parametrize("apod", [("uniform", 0.8, 0.0), ("maxangle", 30.0, 0.0), ("piecewise", 40.0, 20.0)])
def test_a_trivial_medium_gives_kernel_4s_map(apod):
    s = scene()
    xs, ys, zs = smo.grid_axes(s["origin"], s["spacing"], s["n"])
    xaxis = np.tile([1.0, 0.0, 0.0], (16, 1)); size = np.tile([2.7e-3, 2.7e-3], (16, 1))
    for directivity in (None, (xaxis, size)):
        ref, na_ref, ex_ref = so.steering_map(xs, ys, zs, s["pos"], s["nrm"], s["area"], F0, C, P0, apod=apod, directivity=directivity)
        for delays in ("straight_ray", "direct"):
            P, na, ex = smo.steering_map_medium(s["origin"], s["spacing"], s["n"], s["pos"], s["nrm"], s["area"], F0, C, P0, apod=apod,
                                                sound_speed=np.full(s["n"], C, np.float32), attenuation=np.zeros(s["n"], np.float32),
                                                delays=delays, directivity=directivity)
            assert np.abs(P - ref).max() <= 1e-14 * ref.max() and np.array_equal(na, na_ref) and np.array_equal(ex, ex_ref)


def test_a_uniform_slab_between_element_and_voxel_has_a_closed_form():
    n, spacing, origin = (5, 5, 12), (1e-3, 1e-3, 0.5e-3), (-2e-3, -2e-3, 1e-3)
    pos = np.array([[0.3e-3, -0.2e-3, 0.0]])
    att = np.zeros(n, dtype=np.float32)
    m, a_db = 4, 6.0
    att[:, :, 3:3 + m] = a_db
    a = float(mao.np_per_m(np.float32(a_db), F0))
    A, E = smo.medium_sums(origin, spacing, n, pos, F0, C, None, att)
    A = A.reshape(n + (1,))
    xs, ys, zs = smo.grid_axes(origin, spacing, n)
    for (i, j, k) in [(0, 0, 9), (4, 2, 11), (2, 2, 8), (1, 3, 7)]:          # voxels above the slab (planes 3 .. 6)
        w = np.array([xs[i], ys[j], zs[k]]) - pos[0]
        assert A[i, j, k, 0] == pytest.approx(spacing[2] * np.linalg.norm(w) / abs(w[2]) * m * a, rel=1e-13)
    assert np.all(A[:, :, :3] == 0) and np.all(E == 0)
    w = np.array([xs[2], ys[2], zs[4]]) - pos[0]                              # inside the slab: plane 3 crossed, half of the voxel's own plane 4
    assert A[2, 2, 4, 0] == pytest.approx(spacing[2] * np.linalg.norm(w) / abs(w[2]) * 1.5 * a, rel=1e-13)


def test_equalize_without_spreading_is_hmin_times_the_uncompensated_water_sum():
    s = scene()
    apod = ("maxangle", 35.0, 0.0)
    sums = smo.medium_sums(s["origin"], s["spacing"], s["n"], s["pos"], F0, C, s["ss"], s["att"])
    P, na, _ = smo.steering_map_medium(s["origin"], s["spacing"], s["n"], s["pos"], s["nrm"], s["area"], F0, C, P0, apod=apod, sound_speed=s["ss"],
                                       attenuation=s["att"], comp="equalize", sums=sums)
    xs, ys, zs = smo.grid_axes(s["origin"], s["spacing"], s["n"])
    water, _, _ = so.steering_map(xs, ys, zs, s["pos"], s["nrm"], s["area"], F0, C, P0, apod=apod)       # (P0 / lambda) sum b S / d'
    X, Y, Z = np.meshgrid(xs, ys, zs, indexing="ij")
    w = np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1)[:, None, :] - s["pos"][None, :, :]
    b = smo.base_apodization(w, s["nrm"] / np.linalg.norm(s["nrm"], axis=1)[:, None], apod)
    hmin = np.where(b > 0, np.exp(-sums[0]), np.inf).min(axis=1)
    hmin[~(b > 0).any(axis=1)] = 0.0
    assert (na == 0).any() and (na > 0).any()
    assert np.abs(P.ravel() - hmin * water.ravel()).max() <= 1e-13 * P.max()
    matched, _, _ = smo.steering_map_medium(s["origin"], s["spacing"], s["n"], s["pos"], s["nrm"], s["area"], F0, C, P0, apod=apod, sound_speed=s["ss"],
                                            attenuation=s["att"], comp="matched", sums=sums)
    plain, _, _ = smo.steering_map_medium(s["origin"], s["spacing"], s["n"], s["pos"], s["nrm"], s["area"], F0, C, P0, apod=apod, sound_speed=s["ss"],
                                          attenuation=s["att"], sums=sums)
    assert np.all(P <= plain + 1e-9 * P.max()) and np.all(matched <= plain + 1e-9 * P.max())         # c_e <= b_e in both modes
    direct, _, _ = smo.steering_map_medium(s["origin"], s["spacing"], s["n"], s["pos"], s["nrm"], s["area"], F0, C, P0, apod=apod, sound_speed=s["ss"],
                                           attenuation=s["att"], delays="direct", sums=sums)
    assert np.all(direct <= plain + 1e-9 * P.max()) and direct.sum() < 0.99 * plain.sum()             # the residual phase costs pressure


# ---- the Python argument handling, engine stubbed ------------------------------------------------------------------------
class FakeEngine:
    def __init__(self, volumes):
        self.calls, self.volumes = [], list(volumes)

    def steering_map(self, arr, origin_m, spacing_m, n, freq, c, p0_pa, apod=None, absorption=0.0, directivity=False, medium=None):
        self.calls.append(dict(n=tuple(int(v) for v in n), freq=freq, c=c, p0_pa=p0_pa, apod=apod, absorption=absorption, directivity=directivity,
                               medium=medium))
        shape = tuple(int(v) for v in n)
        return self.volumes.pop(0).reshape(shape).astype(np.float32), np.full(shape, 4, dtype=np.int32)


def small_params(het=False, att=0.0):
    setup = ol.SimSetup(spacing=1.0, x_extent=(-3, 3), y_extent=(-3, 3), z_extent=(5, 11))
    params = setup.setup_sim_scene(ol.seg.seg_methods.UniformWater())
    if att:
        a = np.full(np.asarray(params["attenuation"].data).shape, att, dtype=np.float32)
        params["attenuation"] = ds.make_dataarray(a, coords=params.coords, dims=list(params.coords.keys()), name="attenuation",
                                                  attrs=dict(params["attenuation"].attrs))
    if het:
        c = np.array(params["sound_speed"].data, dtype=np.float32)
        c[2, 2, 3:] = 2800.0
        params["sound_speed"] = ds.make_dataarray(c, coords=params.coords, dims=list(params.coords.keys()), name="sound_speed",
                                                  attrs=dict(params["sound_speed"].attrs))
    return params


def test_python_argument_handling(monkeypatch):
    arr = ol.Transducer.gen_matrix_array(nx=2, ny=2, pitch=3, kerf=0.3, units="mm")
    arr.frequency = F0
    shape = (7, 7, 7)
    V = int(np.prod(shape))
    p = np.linspace(1.0, 2.0, V); p[0] = 0.0; p[1] = 0.0
    pw = np.full(V, 2.0); pw[0] = 0.0
    fake = FakeEngine([])
    monkeypatch.setattr(steering_mod, "get_engine", lambda: fake)
    # the default mode is today's function: both refusals stand, nothing reaches the engine
    with pytest.raises(NotImplementedError, match="MediumCompensated"):
        calc_steering_map(arr, small_params(), apod_method=ol.apod_methods.MediumCompensated())
    with pytest.raises(NotImplementedError, match="heterogeneous"):
        calc_steering_map(arr, small_params(het=True), freq=F0)
    with pytest.raises(ValueError, match="medium_model"):
        calc_steering_map(arr, small_params(het=True), medium_model="marched")
    with pytest.raises(NotImplementedError, match="delay method"):
        calc_steering_map(arr, small_params(het=True), medium_model="straight_ray", delay_method=object())
    assert fake.calls == []
    # a homogeneous medium with a plain apodization still runs kernel 4 (the scene's uniform attenuation as exp(-alpha d)); water = absorption 0
    fake.volumes = [p.copy(), pw.copy()]
    base = ol.apod_methods.MaxAngle(max_angle=30.0)
    sm = calc_steering_map(arr, small_params(att=0.5), apod_method=base, medium_model="straight_ray")
    assert [c["medium"] for c in fake.calls] == [None, None] and fake.calls[0]["absorption"] > 0 and fake.calls[1]["absorption"] == 0.0
    assert fake.calls[0]["apod"] == base.kernel_args() == fake.calls[1]["apod"]
    g = np.asarray(sm.dataset["medium_gain_db"].data).ravel()
    assert np.isnan(g[0]) and g[1] == -np.inf and g[-1] == 0.0 and g[2] == pytest.approx(20 * np.log10(p[2] / 2.0), abs=1e-5)
    assert sm.dataset["medium_gain_db"].attrs["units"] == "dB"
    assert np.array_equal(sm.envelope(-3.0), np.asarray(sm.dataset["steering_gain_db"].data) >= -3.0)
    # a heterogeneous medium runs kernel 4h, StraightRay by default, Direct on request
    fake.calls.clear(); fake.volumes = [p.copy(), pw.copy(), p.copy(), pw.copy()]
    het = small_params(het=True)
    calc_steering_map(arr, het, apod_method=base, medium_model="straight_ray", directivity=True)
    calc_steering_map(arr, het, apod_method=base, medium_model="straight_ray", delay_method=ol.delay_methods.Direct())
    m0, m2 = fake.calls[0]["medium"], fake.calls[2]["medium"]
    assert m0["delays"] == "straight_ray" and m2["delays"] == "direct" and m0["comp"] is None and m0["spreading"] is False
    assert m0["sound_speed"].dtype == np.float32 and m0["sound_speed"][2, 2, 3] == 2800.0 and fake.calls[0]["absorption"] == 0.0
    assert fake.calls[1]["medium"] is None and fake.calls[1]["absorption"] == 0.0 and fake.calls[1]["directivity"] is True
    assert fake.calls[0]["c"] == float(het["sound_speed"].attrs["ref_value"])
    # MediumCompensated unpacked into base / mode / spreading / frequency; it selects kernel 4h in a homogeneous medium too
    fake.calls.clear(); fake.volumes = [p.copy(), pw.copy(), p.copy(), pw.copy()]
    mc = ol.apod_methods.MediumCompensated(base=base, mode="matched", spreading=True, frequency=300e3)
    calc_steering_map(arr, small_params(att=0.5), apod_method=mc, medium_model="straight_ray")
    m = fake.calls[0]["medium"]
    assert fake.calls[0]["apod"] == base.kernel_args() and m["comp"] == "matched" and m["spreading"] is True and m["sound_speed"] is None
    assert m["attenuation"].dtype == np.float32 and np.allclose(m["attenuation"], 0.5 * (300e3 / F0) ** 0.9, rtol=1e-6) and fake.calls[0]["freq"] == F0
    proto = ol.Protocol(pulse=ol.Pulse(frequency=F0, amplitude=0.5, duration=2e-5), apod_method=ol.apod_methods.MediumCompensated(mode="equalize"),
                        delay_method=ol.delay_methods.Direct())
    proto.calc_steering_map(arr, het, medium_model="straight_ray")
    m = fake.calls[2]["medium"]
    assert m["comp"] == "equalize" and m["delays"] == "direct" and fake.calls[2]["p0_pa"] == 0.5 and fake.calls[3]["medium"] is None
    # the default call of the Protocol is unchanged: one kernel-4 call, no medium_gain_db
    fake.calls.clear(); fake.volumes = [p.copy()]
    sm = ol.Protocol(pulse=ol.Pulse(frequency=F0, duration=2e-5)).calc_steering_map(arr, small_params())
    assert len(fake.calls) == 1 and fake.calls[0]["medium"] is None and "medium_gain_db" not in sm.dataset
