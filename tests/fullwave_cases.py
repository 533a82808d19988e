"""Case table of the full-wave parity tests (tests/test_gpu_fullwave.py): each case is the input of ONE run on the grid the device sees
(absorbing layers included), handed unchanged to the C-ABI and to the fp64 oracle (tests/fullwave_oracle.py).  Oracle results are
computed once per case and shared."""
import functools

import numpy as np

import fullwave_oracle as fo

FREQ = 500e3
WATER = (1500.0, 1000.0, 0.0)          # c [m/s], rho [kg/m^3], alpha [Np/m at FREQ]
SKULL = (2800.0, 1900.0, 37.0)
TISSUE = (1560.0, 1050.0, 1.85)
INCLUSION_C = 2200.0


def layered(n):
    """water / skull / tissue along z with a 2200 m/s inclusion inside the skull -> (c, rho, alpha) volumes"""
    nz = n[2]
    lab = np.zeros(n, dtype=int)
    lab[..., nz // 3: nz // 2] = 1
    lab[..., nz // 2:] = 2
    mats = np.array([WATER, SKULL, TISSUE])
    c, rho, alpha = (mats[lab, q].copy() for q in range(3))
    c[n[0] // 3: n[0] // 3 + 4, n[1] // 3: n[1] // 3 + 5, nz // 3 + 1: nz // 2 - 1] = INCLUSION_C
    return c, rho, alpha


def bound(h, c_max):
    h = np.broadcast_to(np.asarray(h, dtype=np.float64), (3,))
    return 6.0 / (7.0 * c_max * np.sqrt(np.sum(1.0 / h ** 2)))


def _case(n, h, medium, pml, pos_vox, A, tau_steps, steps, cycles=3.0, ramp=0.0, frac_dt=0.9, pml_alpha=2.0, trace=()):
    """pos_vox: element positions in voxel units of the grid; tau_steps: delays in units of dt (chosen off the half-integers)."""
    c, rho, alpha = medium
    dt = frac_dt * bound(h, float(np.max(c)))
    hh = np.broadcast_to(np.asarray(h, dtype=np.float64), (3,))
    tau = np.asarray(tau_steps, dtype=np.float64) * dt
    ijk, amp, tt = fo.monopole_entries(np.asarray(pos_vox, dtype=np.float64) * hh, (0, 0, 0), hh, A, tau, c, FREQ, dt, n)
    return dict(n=tuple(n), h=tuple(hh), c=c, rho=rho, alpha=alpha, c_ref=1500.0, pml=pml, pml_alpha=pml_alpha, dt=dt, steps=steps, ijk=ijk,
                amp=amp, tau=tt, freq=FREQ, cycles=cycles, ramp=ramp, trace=np.asarray(trace, dtype=np.int64).reshape(-1, 3))


def _cases():
    out = {}
    # uniform water, about 32^3, 6-voxel layers; one element on a voxel, one off
    out["uniform_water"] = _case((32, 32, 32), 0.5e-3, WATER, 6, [(12, 15, 9), (17.3, 14.6, 9.25)], [1.0, 0.7], [0.2, 7.3], 300,
                                 trace=[(16, 16, 20), (8, 20, 25), (0, 0, 0)])
    # layered medium with an inclusion on an odd anisotropic grid, all three volumes; bursts that start and end inside the run, a ramp,
    # two elements sharing voxels, an element with apodization 0
    n, h = (37, 29, 43), (0.4e-3, 0.5e-3, 0.3e-3)
    pos = [(12.4, 9.7, 8.2), (12.6, 9.2, 8.9), (24.0, 18.0, 8.0), (20.5, 12.5, 9.5), (8.3, 20.1, 7.7)]
    A = [1.0, 0.8, 0.6, 0.0, 0.9]
    tau = [0.3, 11.7, 25.2, 3.3, 40.8]
    out["layered"] = _case(n, h, layered(n), 6, pos, A, tau, 400, cycles=2.5, ramp=0.0, trace=[(18, 14, 30), (13, 10, 16), (36, 28, 42)])
    out["layered_ramp"] = _case(n, h, layered(n), 6, pos, A, tau, 400, cycles=4.0, ramp=1.5, trace=[(18, 14, 30)])
    c, rho, alpha = layered(n)
    out["lossless"] = _case(n, h, (c, rho, 0.0), 0, pos, A, tau, 300, trace=[(18, 14, 30)])
    out["absorbing_only"] = _case(n, h, (WATER[0], WATER[1], alpha), 6, pos, A, tau, 300, trace=[(18, 14, 30)])
    out["density_only"] = _case(n, h, (WATER[0], rho, 0.0), 6, pos, A, tau, 200)
    # an axis of 5 voxels (shorter than two stencil reaches), no layers; sources in voxels 0 / 1 and n - 2 / n - 1 of the axes
    n5 = (5, 21, 23)
    out["short_axis"] = _case(n5, 0.5e-3, WATER, 0, [(0.4, 0.5, 0.5), (3.6, 19.5, 21.5), (2, 10, 11)], [1.0, 1.0, 0.5], [0.2, 3.4, 9.1], 200,
                              trace=[(0, 0, 0), (4, 20, 22), (2, 10, 12)])
    c5, rho5, a5 = layered(n5)
    out["short_axis_layered"] = _case(n5, (0.5e-3, 0.4e-3, 0.3e-3), (c5, rho5, a5), 0, [(0.4, 0.5, 0.5), (3.6, 19.5, 21.5)], [1.0, 1.0], [0.2, 3.4], 200,
                                      trace=[(0, 0, 0), (4, 20, 22)])
    return out


CASES = _cases()


@functools.lru_cache(maxsize=None)
def reference(name):
    k = CASES[name]
    ref = fo.simulate(k["n"], k["h"], k["c"], k["rho"], k["alpha"], k["c_ref"], k["pml"], k["pml_alpha"], k["dt"], k["steps"], k["ijk"], k["amp"],
                      k["tau"], k["freq"], k["cycles"], k["ramp"], trace_ijk=k["trace"])
    for v in ref.values():
        v.setflags(write=False)
    return ref


def lin(ijk, n):
    ijk = np.asarray(ijk, dtype=np.int64).reshape(-1, 3)
    return (ijk[:, 0] * n[1] + ijk[:, 1]) * n[2] + ijk[:, 2]


def run_device(ctx, name, split=None, psq=True):
    """The case through the C-ABI -> (p_max, p_min, psq, trace [steps, P])."""
    k = CASES[name]
    ctx.fullwave_plan(k["h"], k["n"], k["c"], k["rho"], k["alpha"], k["c_ref"], k["pml"], k["pml_alpha"], k["dt"])
    ctx.fullwave_sources(lin(k["ijk"], k["n"]), k["amp"], k["tau"], k["freq"], k["cycles"], k["ramp"], k["steps"], points=lin(k["trace"], k["n"]))
    if split is None:
        ctx.fullwave_run(0, k["steps"], psq=psq)
    else:
        ctx.fullwave_run(0, split, psq=psq)
        ctx.fullwave_run(split, k["steps"] - split, psq=psq)
    return ctx.fullwave_fetch()


def deviations(got, ref):
    """largest deviation of each record as a fraction of that record's maximum in the oracle"""
    pmax, pmin, psq, tr = got
    out = {}
    for key, g in (("p_max", pmax), ("p_min", pmin), ("psq", psq), ("trace", tr)):
        r = ref[key]
        if g is None or r.size == 0:
            continue
        scale = np.abs(r).max()
        assert scale > 0, key
        out[key] = float(np.abs(g.astype(np.float64) - r).max() / scale)
    return out
