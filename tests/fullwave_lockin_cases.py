"""Scenes of the lock-in and TimeReversal tests, shared by tests/test_fullwave_lockin_host.py (oracle only) and
tests/test_gpu_fullwave_lockin.py (device against oracle).  Oracle results are computed once and shared.

The array scene is that of ``focus_deviation`` in tests/test_fullwave_host.py: a 4 x 4 array, pitch 1.5 mm, elements off the voxels, a
voxel focus 4.5 mm deep, 500 kHz, absorbing layers of 12 voxels, cfl 0.3 -- in water, or with a wedge-shaped skull slab between array and
focus (c = 2800 m/s, rho = 1900 kg/m^3, 40 Np/m, thickness 1.6 mm + 0.4 x)."""
import functools

import numpy as np

import fullwave_cases as fc
import fullwave_lockin_oracle as lo
import fullwave_oracle as fo
import medium_delay_oracle as mo

F0, C0, RHO = 500e3, 1500.0, 1000.0
SKULL = (2800.0, 1900.0, 40.0)
RAMP, SETTLE, LOCKIN = 2.0, 3.0, 4.0


def array_scene(h, medium="water", pml=12, half_mm=3.6, depth_mm=6.0, pitch=1.5e-3, focus_depth=4.5e-3, slab=(0.75e-3, 1.6e-3, 0.4)):
    """dict(n, h, c, rho, alpha, pos [16, 3] m, focus [3] m, focus_ijk, dt, pml): the whole grid (layers included), voxel 0 at the origin.
    ``slab = (distance from the array, thickness at x = 0, slope of the thickness in x)`` of the wedge."""
    half = int(round(half_mm * 1e-3 / h))
    nz = int(round(depth_mm * 1e-3 / h))
    n = (2 * half + 1 + 2 * pml, 2 * half + 1 + 2 * pml, nz + 2 * pml)
    ctr = np.array([(pml + half) * h, (pml + half) * h, (pml + 1.5) * h])
    g = (np.arange(4) - 1.5) * pitch
    pos = np.array([[ctr[0] + x + 0.2 * h, ctr[1] + y + 0.35 * h, ctr[2]] for x in g for y in g])
    kf = int(round((ctr[2] + focus_depth) / h))
    focus_ijk = np.array([pml + half, pml + half, kf])
    c, rho, alpha = np.full(n, C0), np.full(n, RHO), np.zeros(n)
    if medium == "wedge":
        x = np.clip(np.arange(n[0]) * h - ctr[0], -half * h, half * h)
        z = np.arange(n[2]) * h
        z0 = ctr[2] + slab[0]
        inside = (z[None, :] >= z0) & (z[None, :] < z0 + slab[1] + slab[2] * x[:, None])          # [nx, nz]
        m = np.broadcast_to(inside[:, None, :], n)
        c[m], rho[m], alpha[m] = SKULL
    elif medium != "water":
        raise ValueError(medium)
    return dict(n=n, h=h, c=c, rho=rho, alpha=alpha, pos=pos, focus=focus_ijk * h, focus_ijk=focus_ijk, dt=0.3 * h / float(c.max()), pml=pml, half=half)


def small_wedge():
    """The wedge scene shrunk for the device test: pitch 1 mm, focus 7 voxels deep, layers of 6 voxels, the slab 0.9 mm + 0.3 x thick"""
    return array_scene(0.375e-3, "wedge", pml=6, half_mm=2.25, depth_mm=3.375, pitch=1.0e-3, focus_depth=2.625e-3, slab=(0.375e-3, 0.9e-3, 0.3))


def time_axis(sc, settle=SETTLE, lockin=LOCKIN, ramp=RAMP, travel=4e-6):
    """(n_steps, cycles, w0, Nw) of a driven run of the scene: t_end = travel + (ramp + settle + lockin) / f0"""
    t_end = travel + (ramp + settle + lockin) / F0
    n_steps = int(np.ceil(t_end / sc["dt"]))
    w0, nw = lo.window_of(n_steps, sc["dt"], F0, lockin)
    return n_steps, lo.drive_cycles(F0, t_end), w0, nw


def _run(sc, src, rec_points, axis, extra=(), ramp=RAMP):
    n_steps, cycles, w0, nw = axis
    return lo.steady_receivers(sc["n"], sc["h"], sc["c"], sc["rho"], sc["alpha"], C0, sc["pml"], 2.0, sc["dt"], n_steps, src, rec_points, F0, cycles,
                               ramp, w0, nw, trace_extra=extra)


def listen(sc, axis, ramp=RAMP):
    """The time-reversal run: a unit monopole at the focus, the elements listen -> Z [16]"""
    src = fo.monopole_entries(sc["focus"][None], (0, 0, 0), sc["h"], [1.0], [0.0], sc["c"], F0, sc["dt"], sc["n"])
    return _run(sc, src, sc["pos"], axis, ramp=ramp)[0]


def fire(sc, delays, axis):
    """The forward run: the array fires with ``delays`` -> steady amplitude at the focus voxel"""
    A = np.full(16, 1e-6 * 1e5 * F0 / C0)
    src = fo.monopole_entries(sc["pos"], (0, 0, 0), sc["h"], A, delays, sc["c"], F0, sc["dt"], sc["n"])
    Z = _run(sc, src, sc["focus"][None], axis)[0]
    return float(2.0 / axis[3] * abs(Z[0]))


def direct_delays(sc):
    d = np.sqrt(((sc["pos"] - sc["focus"]) ** 2).sum(axis=1))
    return (d.max() - d) / C0


def straight_ray_delays(sc):
    return mo.delays(sc["pos"], sc["focus"][None], sc["c"], (0.0, 0.0, 0.0), (sc["h"],) * 3, C0)[0]


@functools.lru_cache(maxsize=None)
def time_reversal_case(medium, h, anchor="straight_ray", settle=SETTLE):
    """(delays, tie margin, Z, anchor delays, axis) of the oracle's TimeReversal on the array scene"""
    sc = array_scene(h, medium)
    axis = time_axis(sc, settle=settle)
    Z = listen(sc, axis)
    d = straight_ray_delays(sc) if anchor == "straight_ray" else direct_delays(sc)
    delays, margin, _, _ = lo.time_reversal(Z, d, F0)
    return delays, margin, Z, d, axis


# ---- the device cases: fullwave_cases' inputs with a full-volume trace, and receiver tables in voxel units --------------------------
LOCK_CASES = ("uniform_water", "layered", "short_axis")


@functools.lru_cache(maxsize=None)
def full_trace(name):
    """p~ of every step at every voxel [steps, voxels] (C order) of a fullwave_cases case"""
    k = fc.CASES[name]
    every = np.stack(np.meshgrid(*[np.arange(v) for v in k["n"]], indexing="ij"), axis=-1).reshape(-1, 3)
    tr = fo.simulate(k["n"], k["h"], k["c"], k["rho"], k["alpha"], k["c_ref"], k["pml"], k["pml_alpha"], k["dt"], k["steps"], k["ijk"], k["amp"],
                     k["tau"], k["freq"], k["cycles"], k["ramp"], trace_ijk=every)["trace"]
    tr.setflags(write=False)
    return tr


def receivers(name, many=70, seed=11):
    """Receiver positions in voxel units of a case's grid: on a voxel (1 entry), off it (8), in voxels 0 / 1 and n - 2 / n - 1 of every
    axis, two sharing voxels, and random ones up to ``many`` (more than one wave of 64) -> [R, 3]"""
    n = np.asarray(fc.CASES[name]["n"], dtype=np.float64)
    pts = [np.floor(n / 2), np.floor(n / 2) + (0.3, 0.45, 0.6), (0.4, 0.5, 0.25), n - 1 - (0.4, 0.5, 0.25), np.floor(n / 3) + (0.5, 0.5, 0.5),
           np.floor(n / 3) + (0.25, 0.75, 0.5), (0.0, 0.0, 0.0), n - 1]
    rng = np.random.default_rng(seed)
    while len(pts) < many:
        pts.append(rng.uniform(0, 1, 3) * (n - 1))
    return np.asarray(pts, dtype=np.float64)


def receiver_csr(name, points_vox, empty_row_at=3):
    """CSR table of the receivers (linear voxels of the case's grid) with an empty row inserted at ``empty_row_at`` (None: no empty row)"""
    k = fc.CASES[name]
    row, ijk, wt = lo.trilinear(np.asarray(points_vox) * np.asarray(k["h"]), (0, 0, 0), k["h"], k["n"])
    if empty_row_at is not None and empty_row_at < len(row):
        row = np.insert(row, empty_row_at, row[empty_row_at])
    return row.astype(np.int32), fc.lin(ijk, k["n"]), wt


def lockin_reference(name, window, table=None):
    """(C [n], S [n], C_r, S_r) of the oracle for the steps ``window = (w0, Nw)``"""
    k = fc.CASES[name]
    tr = full_trace(name)
    C, S = lo.volume_sums(tr, k["freq"], k["dt"], *window)
    out = [C.reshape(k["n"]), S.reshape(k["n"]), None, None]
    if table is not None:
        row, vox, wt = table
        out[2], out[3] = lo.receiver_sums(tr, {int(v): int(v) for v in vox}, row, vox, wt, k["freq"], k["dt"], *window)
    return tuple(out)


def run_device(ctx, name, window, table=None, volume=True, psq=True, split=None):
    """The case with a lock-in through the C-ABI -> ((p_max, p_min, psq, trace), (C, S, C_r, S_r))"""
    k = fc.CASES[name]
    ctx.fullwave_plan(k["h"], k["n"], k["c"], k["rho"], k["alpha"], k["c_ref"], k["pml"], k["pml_alpha"], k["dt"])
    ctx.fullwave_sources(fc.lin(k["ijk"], k["n"]), k["amp"], k["tau"], k["freq"], k["cycles"], k["ramp"], k["steps"], points=fc.lin(k["trace"], k["n"]))
    row, vox, wt = (None, None, None) if table is None else table
    ctx.fullwave_lockin(k["freq"], window[0], window[1], volume=volume, row=row, voxels=vox, weights=wt)
    if split is None:
        ctx.fullwave_run(0, k["steps"], psq=psq)
    else:
        ctx.fullwave_run(0, split, psq=psq)
        ctx.fullwave_run(split, k["steps"] - split, psq=psq)
    return ctx.fullwave_fetch(), ctx.fullwave_fetch_lockin()


def deviations(got, ref):
    """Largest deviation of the volume sums as a fraction of the oracle's max hypot(C, S), of the receiver sums as a fraction of the
    largest |Z_r|"""
    out = {}
    if got[0] is not None:
        scale = np.hypot(ref[0], ref[1]).max()
        assert scale > 0
        out["volume"] = float(max(np.abs(got[0] - ref[0]).max(), np.abs(got[1] - ref[1]).max()) / scale)
    if got[2] is not None:
        scale = np.hypot(ref[2], ref[3]).max()
        assert scale > 0
        out["receivers"] = float(max(np.abs(got[2] - ref[2]).max(), np.abs(got[3] - ref[3]).max()) / scale)
    return out
