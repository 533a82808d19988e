"""Rectangular element apertures of the full-wave model, host side (no GPU): the fp64 oracle of the weights
(tests/fullwave_aperture_oracle.py) against the properties of the definition, the product's host halves (quadrature counts, points,
refusals -- every one raised before any device call) and the directivity known answer on the oracle of the scheme.

Directivity scene: 72 x 20 x 56 voxels of 0.5 mm inside 8-voxel layers, water at 1500 m/s, 500 kHz, dt = 0.3 h / c,
313 steps (ramp 2 cycles, lock-in over the last 4 cycles); one 6 x 1 mm element (2 wavelengths wide, first null at 30 degrees), normal
+z, centre at voxel (36, 10, 5.3), rate 5: 78 entries.  The amplitude at the voxels nearest 20 mm from the centre at 0 .. 50 degrees in
the xz plane, as a fraction of the on-axis value, against |sum e^{ikr} / r| / N over a 240 x 40 subdivision of the rectangle: the
aperture model deviates by at most 0.052 of the on-axis value (gate 0.06); one monopole radiates 0.98 of its on-axis value into the
null (gate: a deviation >= 0.5 at 30 degrees)."""
import functools

import numpy as np
import pytest

import openlifu_amd as ol
from openlifu_amd.sim import fullwave as fw
import fullwave_aperture_cases as ac
import fullwave_aperture_oracle as ao
import fullwave_oracle as fo

Z3 = (0.0, 0.0, 0.0)
EX, EY = np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0])


# ---- the oracle against the definition ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["axis_aligned", "tilted", "edges", "many_65"])
def test_weights_sum_to_one(name):
    k = ac.CASES[name]
    row, ijk, wt = ac.weights(name)
    assert row[-1] == wt.size and np.all(wt > 0)
    for e in range(row.size - 1):
        npts = int(k["nw"][e]) * int(k["nl"][e])
        assert abs(wt[row[e]:row[e + 1]].sum() - 1.0) <= 4 * npts * 2.0 ** -53 + 8 * 2.0 ** -53, (name, e)


def test_case_table_is_what_it_says():
    k = ac.CASES["axis_aligned"]
    assert [(int(a), int(b)) for a, b in zip(k["nw"], k["nl"])] == [(15, 25), (30, 5), (2, 2), (1, 1)]
    row, ijk, wt = ac.weights("axis_aligned")
    assert set(ijk[row[1]:row[2], 2]) == {9}                                  # exactly on a plane: the snap gives one plane
    assert row[4] - row[3] == 1 and tuple(ijk[row[3]]) == (22, 12, 9) and wt[row[3]] == 1.0      # one point on a voxel: one entry
    row, ijk, wt = ac.weights("edges")
    assert {0, 4} <= set(ijk[row[0]:row[1], 0])
    assert {19, 20} <= set(ijk[row[1]:row[2], 1]) and {21, 22} <= set(ijk[row[1]:row[2], 2])
    row, ijk, wt = ac.weights("tilted")
    shared = {tuple(m) for m in ijk[row[0]:row[1]]} & {tuple(m) for m in ijk[row[1]:row[2]]}
    assert len(shared) >= 4                                                     # two adjacent elements share border voxels
    assert ac.CASES["tilted"]["A"][2] == 0.0 and ac.CASES["tilted"]["ramp"] > 0
    for name in ("many_1", "many_65", "many_257"):
        assert np.all(ac.CASES[name]["nw"] * ac.CASES[name]["nl"] == 1)
    for name, k in ac.CASES.items():
        assert fo.activity_margin(k["tau"], k["cycles"] / k["freq"], k["dt"]) >= 0.05, name
        assert 200 <= k["steps"] <= 400


def test_one_point_aperture_is_the_point_rule_exactly():
    n, h = (37, 29, 43), np.array([0.4e-3, 0.5e-3, 0.3e-3])
    c, _, _ = ac.fc.layered(n)
    pos = np.array([(12.4, 9.7, 8.2), (24.0, 18.0, 8.0), (20.5, 12.5, 9.5), (8.3, 20.1, 7.7)]) * h
    A, tau, dt = np.array([1.0, 0.6, 0.3, 0.9]), np.array([1e-7, 2e-7, 0.0, 3e-7]), 3e-8
    ang = (0.3, -0.2, 0.5)
    R = ao.rotation(*ang)
    E = len(pos)
    row, ijk, wt = ao.aperture_table(pos, [R[:, 0]] * E, [R[:, 1]] * E, [(0.1e-3, 0.05e-3)] * E, [1] * E, [1] * E, Z3, h, n)
    got = ao.expand(row, ijk, wt, A, tau, c, 500e3, dt, h, n)
    ref = fo.monopole_entries(pos, Z3, h, A, tau, c, 500e3, dt, n)
    for g, r in zip(got, ref):          # (the point rule lists an element's corners in C order, as the CSR does)
        assert np.array_equal(g, r)
    # the product's point rule gives the same entries
    p_ijk, p_w, p_el = fw.trilinear_entries(pos, Z3, h, n)
    assert np.array_equal(p_ijk, ijk) and np.array_equal(p_w, wt) and np.array_equal(np.diff(row), np.bincount(p_el))


def test_a_whole_voxel_shift_moves_the_indices_only():
    n, h = (40, 40, 40), np.array([0.4e-3, 0.5e-3, 0.3e-3])
    R = ao.rotation(0.2, 0.1, -0.4)
    centre = np.array([15.3, 14.6, 12.25]) * h
    shift = np.array([3, -2, 5])
    a = ao.aperture_table([centre], [R[:, 0]], [R[:, 1]], [(1.3e-3, 0.9e-3)], [7], [5], Z3, h, n)
    b = ao.aperture_table([centre], [R[:, 0]], [R[:, 1]], [(1.3e-3, 0.9e-3)], [7], [5], -shift * h, h, n)
    assert np.array_equal(a[1] + shift, b[1])
    # q moves by a whole number up to the rounding of (x - origin) / h: a few ulp of q ~ 20, times the 35 points' unit slopes
    assert np.abs(a[2] - b[2]).max() <= 64 * 2.0 ** -52 * 20


def test_rotation_is_the_products():
    from openlifu_amd.xdc.element import rotation_from_angles
    for ang in [(0.0, 0.0, 0.0), (0.3, -0.2, 0.5), (np.radians(15), np.radians(-10), np.radians(30))]:
        assert np.allclose(ao.rotation(*ang), rotation_from_angles(*ang), rtol=0, atol=1e-15)


# ---- the product's host halves ------------------------------------------------------------------------------------------------------
def _array(**kw):
    return ol.Transducer.gen_matrix_array(nx=2, ny=2, pitch=3.0, kerf=0.5, units="mm", sensitivity=1e5, **kw)


def _params(spacing=0.5, extent=6.0):
    setup = ol.SimSetup(spacing=spacing, x_extent=(-extent, extent), y_extent=(-extent, extent), z_extent=(-2, 10))
    return setup.setup_sim_scene(ol.seg_methods.UniformWater())


def test_geometry_counts_and_points_follow_the_definition():
    arr = _array()
    h = (0.5e-3, 0.4e-3, 0.25e-3)
    geom = fw.aperture_geometry(arr, h, 3)
    size = np.array([[2.5e-3, 2.5e-3]] * 4)
    assert np.allclose(geom["size"], size, rtol=1e-15) and np.allclose(geom["u"], EX) and np.allclose(geom["v"], EY)
    assert np.array_equal(geom["centre"], arr.element_table()[0])
    for e in range(4):
        assert (int(geom["n_w"][e]), int(geom["n_l"][e])) == ao.counts(geom["size"][e], h, 3) == (30, 30)
        q = ao.points_q(geom["centre"][e], geom["u"][e], geom["v"][e], geom["size"][e], 30, 30, Z3, (1.0, 1.0, 1.0))
        assert np.allclose(fw.aperture_points(geom, e), q, rtol=0, atol=1e-18)
    assert fw.aperture_counts([[0.2e-3, 0.1e-3]], 0.5e-3, 5)[0][0] == 2 and fw.aperture_counts([[0.2e-3, 0.1e-3]], 0.5e-3, 5)[1][0] == 1
    assert [int(v[0]) for v in fw.aperture_counts([[0.0, 1e-3]], 0.5e-3, 1)] == [1, 2]
    # a transform moves the centre and turns the axes
    M = np.eye(4); M[:3, :3] = ao.rotation(0.0, 0.0, np.pi / 2); M[:3, 3] = (1e-3, 2e-3, 3e-3)
    g2 = fw.aperture_geometry(arr, h, 3, transform=M)
    assert np.allclose(g2["u"], EY, atol=1e-15) and np.allclose(g2["v"], -EX, atol=1e-15)
    assert np.allclose(g2["centre"], geom["centre"] @ M[:3, :3].T + M[:3, 3])


def test_refusals_come_before_any_device_call(monkeypatch):
    from openlifu_amd.sim import fullwave as mod

    def no_device():
        raise AssertionError("the device was asked for")

    monkeypatch.setattr(mod, "get_engine", no_device)
    arr, params = _array(), _params()
    for run in (fw.run_fullwave_simulation, fw.run_fullwave_steady_state):
        with pytest.raises(ValueError, match="element_model must be one of"):
            run(arr, params, freq=500e3, element_model="piston")
        for rate in (0, -1, 2.5, True):
            with pytest.raises(ValueError, match="upsampling_rate must be an integer >= 1"):
                run(arr, params, freq=500e3, element_model="aperture", upsampling_rate=rate)
        with pytest.raises(ValueError, match="quadrature points"):
            run(arr, params, freq=500e3, element_model="aperture", upsampling_rate=60)      # 2.5 mm at 0.5 mm, rate 60: 300 x 300 points
        # an element half a voxel outside the grid is named: the 4 elements stand at x, y = +-1.5 mm; a grid that ends at 2.5 mm holds the
        # points of the first (x = -1.5 mm: its rectangle reaches -2.75 mm) only to half a voxel short
        small = _params(extent=2.5)
        with pytest.raises(ValueError, match=r"element 0 at .* does not lie inside the grid"):
            run(arr, small, freq=500e3, element_model="aperture", upsampling_rate=5)
    with pytest.raises(ValueError, match="element_model must be one of"):
        ol.bf.delay_methods.TimeReversal(element_model="piston")
    with pytest.raises(ValueError, match="upsampling_rate must be an integer >= 1"):
        ol.bf.delay_methods.TimeReversal(element_model="aperture", upsampling_rate=0)


def test_the_entry_points_take_the_element_model_beside_their_advertised_signatures():
    """The signatures that inspect reports stay the ones the older host tests pin; the element-model keywords are accepted beside them,
    keyword-only, with the defaults of the point model."""
    import inspect
    for fn, extra in ((fw.run_fullwave_simulation, {"element_model": "point"}), (fw.run_fullwave_steady_state, {"element_model": "point", "upsampling_rate": 5})):
        shown = inspect.signature(fn).parameters
        assert not set(extra) & set(shown)
        assert {k: fn.__kwdefaults__[k] for k in extra} == extra
        for k in extra:
            assert k in fn.__doc__
    assert list(inspect.signature(fw.run_fullwave_simulation).parameters)[-1] == "record_points"
    assert list(inspect.signature(fw.run_fullwave_steady_state).parameters)[-1] == "receivers"


def test_point_model_still_ignores_the_rate_and_the_table_refuses_on_the_host(monkeypatch):
    from openlifu_amd.sim import fullwave as mod
    monkeypatch.setattr(mod, "get_engine", lambda: (_ for _ in ()).throw(AssertionError("the device was asked for")))
    geom = fw.aperture_geometry(_array(), 0.5e-3, 5)
    with pytest.raises(ValueError, match="element 0 at .* does not lie inside the grid"):
        fw.aperture_table(geom, (-2.5e-3, -2.5e-3, -1e-3), 0.5e-3, (11, 11, 5))
    assert fw.checked_element_model("point", 5) == ("point", 5)


def test_time_reversal_dict_round_trip():
    TR = ol.bf.delay_methods.TimeReversal
    m = TR(element_model="aperture", upsampling_rate=3)
    d = m.to_dict()
    assert d["class"] == "TimeReversal" and d["element_model"] == "aperture" and d["upsampling_rate"] == 3
    again = ol.bf.delay_methods.DelayMethod.from_dict(d)
    assert isinstance(again, TR) and again == m
    assert ol.bf.delay_methods.DelayMethod.from_dict({"class": "TimeReversal", "element_model": "aperture"}).element_model == "aperture"
    assert TR().element_model == "point" and TR().upsampling_rate == 5


# ---- directivity known answer, on the oracle -----------------------------------------------------------------------------------------
SCENE = dict(n=(72, 20, 56), h=0.5e-3, pml=8, c=1500.0, freq=500e3, steps=313, ramp=2.0, lock=4.0, centre=(36.0, 10.0, 5.3), size=(6e-3, 1e-3), rate=5,
             radius=20e-3, angles=(0, 10, 20, 30, 40, 50))


def scene_points():
    """voxels (of the grid without its layers) nearest ``radius`` from the centre at the angles, in the xz plane"""
    s = SCENE
    return np.array([[int(np.rint(s["centre"][0] + s["radius"] * np.sin(np.radians(a)) / s["h"])), int(s["centre"][1]),
                      int(np.rint(s["centre"][2] + s["radius"] * np.cos(np.radians(a)) / s["h"]))] for a in s["angles"]])


def scene_reference():
    """|sum e^{ikr} / r| / N over a 240 x 40 subdivision of the rectangle at the measured voxels [Pa for A = 1 Pa m]"""
    s = SCENE
    k = 2 * np.pi * s["freq"] / s["c"]
    xs = ((np.arange(240) + 0.5) / 240 - 0.5) * s["size"][0] + s["centre"][0] * s["h"]
    ys = ((np.arange(40) + 0.5) / 40 - 0.5) * s["size"][1] + s["centre"][1] * s["h"]
    X, Y = np.meshgrid(xs, ys, indexing="ij")
    out = []
    for p in scene_points() * s["h"]:
        r = np.sqrt((X - p[0]) ** 2 + (Y - p[1]) ** 2 + (s["centre"][2] * s["h"] - p[2]) ** 2)
        out.append(abs(np.sum(np.exp(1j * k * r) / r)) / X.size)
    return np.array(out)


def scene_entries(model):
    s = SCENE
    h = np.full(3, s["h"])
    dt = 0.3 * s["h"] / s["c"]
    centre = (np.array(s["centre"]) + s["pml"]) * h          # on the grid the scheme sees: the layers lie outside the 72 x 20 x 56 voxels
    npad = tuple(v + 2 * s["pml"] for v in s["n"])
    if model == "aperture":
        nw, nl = ao.counts(s["size"], h, s["rate"])
        row, ijk, wt = ao.aperture_table([centre], [EX], [EY], [s["size"]], [nw], [nl], Z3, h, npad)
        return ao.expand(row, ijk, wt, [1.0], [0.0], s["c"], s["freq"], dt, h, npad)
    return fo.monopole_entries([centre], Z3, h, [1.0], [0.0], s["c"], s["freq"], dt, npad)


def lockin_amplitude(trace, dt, freq, lock_cycles):
    nw = int(np.rint(lock_cycles / (freq * dt)))
    n = np.arange(trace.shape[0] - nw, trace.shape[0])
    ph = freq * (n + 1.0) * dt
    th = 2 * np.pi * (ph - np.floor(ph))
    C, S = (trace[n] * np.cos(th)[:, None]).sum(axis=0), (trace[n] * np.sin(th)[:, None]).sum(axis=0)
    return 2.0 / nw * np.hypot(C, S)


@functools.lru_cache(maxsize=None)
def scene_oracle(model):
    s = SCENE
    dt = 0.3 * s["h"] / s["c"]
    ijk, amp, tau = scene_entries(model)
    ref = fo.simulate(tuple(v + 2 * s["pml"] for v in s["n"]), s["h"], s["c"], 1000.0, 0.0, s["c"], s["pml"], 2.0, dt, s["steps"], ijk, amp, tau, s["freq"],
                      1e3, s["ramp"], trace_ijk=scene_points() + s["pml"])
    return lockin_amplitude(ref["trace"], dt, s["freq"], s["lock"])


def test_directivity_scene_known_answer():
    assert len(scene_entries("aperture")[1]) == 78
    ref = scene_reference()
    print("reference", np.round(ref / ref[0], 4))
    assert ref[3] < 0.15 * ref[0]                            # near the first null at 30 degrees (the nearest voxel is not exactly on it)
    dev = np.abs(scene_oracle("aperture") - ref) / ref[0]
    print("aperture", np.round(dev, 4))
    assert dev.max() <= 0.06
    devp = np.abs(scene_oracle("point") - ref) / ref[0]
    print("point", np.round(devp, 4))
    assert devp[3] >= 0.5
