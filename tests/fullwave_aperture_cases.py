"""Case table of the aperture parity tests (tests/test_gpu_fullwave_aperture.py): each case is the input of ONE run on the grid the
device sees (absorbing layers included, voxel 0 at the origin), handed unchanged to the C-ABI and to the fp64 oracles
(tests/fullwave_aperture_oracle.py for the weights, tests/fullwave_oracle.py for the run).  Delays are in units of dt, off the
half-integers (activity_margin >= 0.05).  Oracle results are computed once per case and shared."""
import functools

import numpy as np

import fullwave_aperture_oracle as ao
import fullwave_cases as fc
import fullwave_oracle as fo

FREQ = fc.FREQ


def _case(n, h, medium, pml, rate, elements, steps, cycles=3.0, ramp=0.0, frac_dt=0.9, trace=()):
    """elements: (centre in voxel units, (w, l) [m], (az, el, roll) [rad], A, tau in units of dt)"""
    c, rho, alpha = medium
    hh = np.broadcast_to(np.asarray(h, dtype=np.float64), (3,)).copy()
    dt = frac_dt * fc.bound(hh, float(np.max(c)))
    centre = np.array([np.asarray(e[0], dtype=np.float64) * hh for e in elements])
    size = np.array([e[1] for e in elements], dtype=np.float64)
    R = [ao.rotation(*e[2]) for e in elements]
    u, v = np.array([r[:, 0] for r in R]), np.array([r[:, 1] for r in R])
    A = np.array([e[3] for e in elements], dtype=np.float64)
    tau = np.array([e[4] for e in elements], dtype=np.float64) * dt
    nw, nl = (np.array(t, dtype=np.int32) for t in zip(*[ao.counts(s, hh, rate) for s in size]))
    return dict(n=tuple(n), h=tuple(hh), c=c, rho=rho, alpha=alpha, c_ref=1500.0, pml=pml, pml_alpha=2.0, dt=dt, steps=steps, freq=FREQ, cycles=cycles,
                ramp=ramp, centre=centre, u=u, v=v, size=size, nw=nw, nl=nl, A=A, tau=tau, trace=np.asarray(trace, dtype=np.int64).reshape(-1, 3))


def _many(n_el):
    """n_el one-point elements (0.1 mm squares at rate 1) on a 7 x 7 x 6 lattice of off-voxel positions inside a 32^3 water grid"""
    els = []
    for e in range(n_el):
        i, j, k = e % 7, (e // 7) % 7, (e // 49) % 6
        els.append(((8.3 + 2.5 * i, 7.6 + 2.5 * j, 8.25 + 2.0 * k), (0.1e-3, 0.1e-3), (0.0, 0.0, 0.0), 0.4 + 0.6 * ((e * 7) % 11) / 10.0, (e % 47) + (0.2, 0.3, 0.4, 0.7, 0.85)[e % 5]))
    return _case((32, 32, 32), 0.5e-3, fc.WATER, 6, 1, els, 200, trace=[(16, 16, 20), (9, 20, 25)])


def _cases():
    out = {}
    z = (0.0, 0.0, 0.0)
    # one general element; one exactly on a plane of voxels (the snap gives one plane); 2 x 2 points around a voxel; one point on a voxel
    out["axis_aligned"] = _case((32, 32, 32), 0.5e-3, fc.WATER, 6, 5,
                                [((12.3, 15.6, 9.25), (1.5e-3, 2.5e-3), z, 1.0, 0.2), ((16.5, 8.5, 9.0), (3.0e-3, 0.5e-3), z, 0.7, 7.3),
                                 ((20.0, 16.0, 9.0), (0.2e-3, 0.2e-3), z, 0.5, 3.4), ((22.0, 12.0, 9.0), (0.1e-3, 0.1e-3), z, 0.6, 12.8)], 300, trace=[(16, 16, 20), (8, 20, 25), (0, 0, 0)])
    # tilted elements on the odd anisotropic layered grid: two adjacent elements sharing border voxels, one with A = 0, different sizes, a ramp
    n, h = (37, 29, 43), (0.4e-3, 0.5e-3, 0.3e-3)
    ang = (np.radians(15.0), np.radians(-10.0), np.radians(30.0))
    R = ao.rotation(*ang)
    c0 = np.array([14.0, 11.0, 9.0])
    c1 = c0 + 1.2e-3 * R[:, 0] / np.array(h)          # one width further along u: the two rectangles share an edge
    out["tilted"] = _case(n, h, fc.layered(n), 6, 3,
                          [(tuple(c0), (1.2e-3, 0.9e-3), ang, 1.0, 0.1), (tuple(c1), (1.2e-3, 0.9e-3), ang, 0.8, 11.7),
                           ((24.0, 18.0, 8.0), (0.7e-3, 1.6e-3), ang, 0.0, 3.8), ((9.3, 20.1, 8.7), (2.0e-3, 0.4e-3), ang, 0.9, 25.15)],
                          400, cycles=4.0, ramp=1.5, trace=[(18, 14, 30), (13, 10, 16), (36, 28, 42)])
    # an axis of 5 voxels, no layers: an element 1.6 mm wide centred at x-voxel 2.0 (its points reach voxels 0 and 4), one reaching n - 2 / n - 1 of y and z
    n5 = (5, 21, 23)
    out["edges"] = _case(n5, 0.5e-3, fc.WATER, 0, 5,
                         [((2.0, 10.3, 11.6), (1.6e-3, 0.6e-3), z, 1.0, 0.2),
                          ((2.5, 19.2, 21.4), (0.4e-3, 0.6e-3), (0.0, np.radians(90.0), 0.0), 0.8, 3.4)], 200, trace=[(0, 0, 0), (4, 20, 22), (2, 10, 12)])
    for n_el in (1, 65, 257):
        out[f"many_{n_el}"] = _many(n_el)
    return out


CASES = _cases()
ORIGIN = (0.0, 0.0, 0.0)


@functools.lru_cache(maxsize=None)
def weights(name):
    """The oracle's per-element CSR (row, ijk, W) of the case"""
    k = CASES[name]
    tab = ao.aperture_table(k["centre"], k["u"], k["v"], k["size"], k["nw"], k["nl"], ORIGIN, k["h"], k["n"])
    for v in tab:
        v.setflags(write=False)
    return tab


@functools.lru_cache(maxsize=None)
def entries(name):
    """The oracle's expanded per-entry table (ijk, amp, tau)"""
    k = CASES[name]
    row, ijk, wt = weights(name)
    return ao.expand(row, ijk, wt, k["A"], k["tau"], k["c"], k["freq"], k["dt"], k["h"], k["n"])


@functools.lru_cache(maxsize=None)
def reference(name):
    k = CASES[name]
    ijk, amp, tau = entries(name)
    ref = fo.simulate(k["n"], k["h"], k["c"], k["rho"], k["alpha"], k["c_ref"], k["pml"], k["pml_alpha"], k["dt"], k["steps"], ijk, amp, tau, k["freq"],
                      k["cycles"], k["ramp"], trace_ijk=k["trace"])
    for v in ref.values():
        v.setflags(write=False)
    return ref


def plan(ctx, name):
    k = CASES[name]
    ctx.fullwave_plan(k["h"], k["n"], k["c"], k["rho"], k["alpha"], k["c_ref"], k["pml"], k["pml_alpha"], k["dt"])


def device_weights(ctx, name, capacity=None):
    """olx_fullwave_apertures on the case's plan -> (row, linear voxels, W)"""
    k = CASES[name]
    plan(ctx, name)
    return ctx.fullwave_apertures(k["centre"], k["u"], k["v"], k["size"], k["nw"], k["nl"], capacity=capacity)


def device_table(ctx, name):
    """The device's weights as the element-factored source table (voxels, elements, amp_{e,m}), formed from the definition"""
    k = CASES[name]
    row, vox, wt = device_weights(ctx, name)
    el = np.repeat(np.arange(row.size - 1), np.diff(row)).astype(np.int32)
    cvol = np.broadcast_to(np.asarray(k["c"], dtype=np.float64), k["n"]).reshape(-1)
    amp = wt * k["dt"] * cvol[vox] ** 2 * 4 * np.pi / (2 * np.pi * k["freq"] * np.prod(k["h"]))
    return vox, el, amp


def run_device(ctx, name, split=None, psq=True, table=None, A=None, tau=None, drive=False):
    """The case through olx_fullwave_apertures and olx_fullwave_sources_elements -> (p_max, p_min, psq, trace [steps, P]).  ``drive``:
    the table goes up with other (A, tau) first and olx_fullwave_drive then sets the case's."""
    k = CASES[name]
    vox, el, amp = device_table(ctx, name) if table is None else table
    A = k["A"] if A is None else A
    tau = k["tau"] if tau is None else tau
    first = (0.5 * A + 0.1, tau + 1.3 * k["dt"]) if drive else (A, tau)
    ctx.fullwave_sources_elements(vox, el, amp, first[0], first[1], k["freq"], k["cycles"], k["ramp"], k["steps"], points=fc.lin(k["trace"], k["n"]))
    if drive:
        ctx.fullwave_drive(A, tau)
    if split is None:
        ctx.fullwave_run(0, k["steps"], psq=psq)
    else:
        ctx.fullwave_run(0, split, psq=psq)
        ctx.fullwave_run(split, k["steps"] - split, psq=psq)
    return ctx.fullwave_fetch()


def run_device_entries(ctx, name, psq=True):
    """The oracle's expanded entries through olx_fullwave_sources (the per-entry form)"""
    k = CASES[name]
    ijk, amp, tau = entries(name)
    plan(ctx, name)
    ctx.fullwave_sources(fc.lin(ijk, k["n"]), amp, tau, k["freq"], k["cycles"], k["ramp"], k["steps"], points=fc.lin(k["trace"], k["n"]))
    ctx.fullwave_run(0, k["steps"], psq=psq)
    return ctx.fullwave_fetch()
