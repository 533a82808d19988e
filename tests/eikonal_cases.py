"""Case table of the eikonal tests, shared by tests/test_gpu_eikonal.py (device against oracle) and its debug-library child process.
The oracle (tests/eikonal_oracle.py) is computed once per case and shared.

Every grid is small -- the kernel can go wrong at rows that are no multiple of the wave, at more than one 256-lane block, at an init ball
clipped by the grid, at fronts that meet behind an inclusion -- not at size."""
import functools

import numpy as np

import eikonal_oracle as eo


def _layered():
    n = (37, 29, 43)
    c = np.full(n, 1500.0, dtype=np.float32)
    c[:, :, 14:22] = 2300.0                   # a fast layer across the grid
    c[:, :, 22:] = 1540.0
    c[6:14, 8:17, 24:32] = 2800.0             # a fast inclusion: the front runs ahead through it
    c[22:31, 10:21, 5:13] = 1000.0            # a slow one: the fronts go round it and meet behind
    return c


H_ISO = (0.5e-3, 0.5e-3, 0.5e-3)
H_ANISO = (0.4e-3, 0.5e-3, 0.3e-3)
ORIGIN = (-3.1e-3, 2.2e-3, 0.7e-3)            # voxel 0 is not at 0: the source's index coordinates are formed from the origin


def _case(n, h, c, q, radius=3.0):
    """q: the source in index coordinates"""
    src = np.asarray(ORIGIN) + np.asarray(q, dtype=np.float64) * np.asarray(h)
    return dict(n=tuple(n), h=tuple(h), origin=ORIGIN, c=c, src=src, radius=float(radius))


CASES = {
    "uniform_water": _case((24, 24, 24), H_ISO, 1500.0, (11.3, 12.45, 9.6)),
    "layered": _case((37, 29, 43), H_ANISO, _layered(), (17.3, 14.6, 2.4)),
    "short_axis": _case((5, 21, 23), H_ISO, 1500.0, (2.2, 9.7, 11.5)),
    "on_voxel": _case((24, 24, 24), H_ISO, 1500.0, (12.0, 11.0, 13.0)),
    "clipped_low": _case((37, 29, 43), H_ANISO, _layered(), (0.4, 1.3, 0.0)),
    "clipped_high": _case((37, 29, 43), H_ANISO, _layered(), (36.0 - 0.4, 28.0 - 1.3, 42.0)),
    "radius_1": _case((24, 24, 24), H_ISO, 1500.0, (12.0, 11.0, 13.0), radius=1.0),
    "radius_5": _case((37, 29, 43), H_ANISO, _layered(), (17.3, 14.6, 2.4), radius=5.0),
}


def lin(ijk, n):
    ijk = np.asarray(ijk, dtype=np.int64)
    return (ijk[:, 0] * int(n[1]) + ijk[:, 1]) * int(n[2]) + ijk[:, 2]


@functools.lru_cache(maxsize=None)
def reference(name):
    """(T [n] fp64, sweeps) of the oracle, from the float32 sound speed the device is given"""
    k = CASES[name]
    c = k["c"] if np.ndim(k["c"]) == 0 else np.asarray(k["c"], dtype=np.float32).astype(np.float64)
    T, sweeps = eo.solve(k["n"], k["origin"], k["h"], c, k["src"], k["radius"])
    T.setflags(write=False)
    return T, sweeps


def points(name, many=71, seed=23):
    """Sample positions [P, 3] in metres: on a voxel (1 entry), off it (8), in voxels 0 / 1 and n - 2 / n - 1 of every axis, two sharing
    voxels, the corner voxels, and random ones up to ``many`` (more than one wave of 64)"""
    k = CASES[name]
    n = np.asarray(k["n"], dtype=np.float64)
    pts = [np.floor(n / 2), np.floor(n / 2) + (0.3, 0.45, 0.6), (0.4, 0.5, 0.25), n - 1 - (0.4, 0.5, 0.25), (1.4, 1.5, 1.25), n - 2 - (0.4, 0.5, 0.25),
           np.floor(n / 3) + (0.5, 0.5, 0.5), np.floor(n / 3) + (0.25, 0.75, 0.5), (0.0, 0.0, 0.0), n - 1]
    rng = np.random.default_rng(seed)
    while len(pts) < many:
        pts.append(rng.uniform(0, 1, 3) * (n - 1))
    return np.asarray(k["origin"]) + np.asarray(pts, dtype=np.float64) * np.asarray(k["h"])


def table(name, pts=None):
    """CSR sample table (row, linear voxel, weight) of the points"""
    k = CASES[name]
    row, ijk, wt = eo.trilinear_table(points(name) if pts is None else pts, k["origin"], k["h"], k["n"])
    return row, lin(ijk, k["n"]), wt


def sample_reference(name, pts=None):
    k = CASES[name]
    return eo.sample(reference(name)[0], eo.trilinear_table(points(name) if pts is None else pts, k["origin"], k["h"], k["n"]))


def run_device(ctx, name, max_sweeps=None):
    """The case through the C-ABI -> (T volume float32, sweeps, T at the sample points float64)"""
    k = CASES[name]
    sweeps = ctx.eikonal_solve(k["origin"], k["h"], k["n"], k["c"], k["src"], init_radius=k["radius"], max_sweeps=max_sweeps)
    return ctx.eikonal_fetch(), sweeps, ctx.eikonal_sample(*table(name))


def deviations(got, name):
    """Largest deviation of the volume and of the samples from the oracle, as fractions of the oracle's largest T"""
    T, _ = reference(name)
    assert np.isfinite(T).all() and T.max() > 0
    vol, _, smp = got
    assert np.isfinite(vol).all()
    return {"volume": float(np.abs(vol.astype(np.float64) - T).max() / T.max()),
            "samples": float(np.abs(smp - sample_reference(name)).max() / T.max())}


# ---- the method's scene A as the product sees it: a Transducer and a params-like object ----------------------------------------------
class Params:
    """The part of a params Dataset the delay methods read: coords (metres) and params["sound_speed"] (data, attrs["ref_value"])."""

    def __init__(self, c, origin, spacing, c_ref, uniform_value=None, n=None):
        """c: the volume, or with ``uniform_value`` the grid's counts; ``n``: counts of the coords when they are not the volume's"""
        from types import SimpleNamespace
        n = n if n is not None else (np.shape(c) if uniform_value is None else c)
        self.coords = {d: SimpleNamespace(data=origin[a] + np.arange(n[a]) * spacing[a], attrs={"units": "m"}) for a, d in enumerate("xyz")}
        if uniform_value is None:
            self._ss = SimpleNamespace(data=c, attrs={"ref_value": c_ref})
        else:
            self._ss = SimpleNamespace(uniform_value=uniform_value, attrs={"ref_value": c_ref})

    def __getitem__(self, key):
        assert key == "sound_speed"
        return self._ss


def array_of(pos_m):
    import openlifu_amd as ol
    els = [ol.Element(index=i + 1, position=p, size=(1e-3, 1e-3), units="m") for i, p in enumerate(np.asarray(pos_m))]
    return ol.Transducer(elements=els, units="m")


@functools.lru_cache(maxsize=None)
def scene_a_method(h=0.5e-3):
    """(scene, params, target Point, the oracle's method result) of scene A.  The oracle is given the grid as the product reads it from the
    coords and the focus as it reads it from the Point, so both decide the init set from the same index coordinates."""
    import openlifu_amd as ol
    from openlifu_amd.engine import focus_positions_m, grid_from_coords
    sc = eo.scene_a(h)
    params = Params(sc["c"], sc["origin"], sc["spacing"], sc["c_ref"])
    origin, spacing, n = grid_from_coords(params.coords)
    assert tuple(n) == sc["n"]
    target = ol.Point(position=tuple(sc["focus"] * 1e3), units="mm")
    ref = eo.method(sc["pos"], focus_positions_m(target)[0], sc["c"].astype(np.float64), origin, spacing, sc["c_ref"])
    return sc, params, target, ref
