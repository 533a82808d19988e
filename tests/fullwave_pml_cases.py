"""Case table of the split-layer parity tests (tests/test_gpu_fullwave_pml.py), built like tests/fullwave_cases.py: each case is the input of
ONE run on the grid the device sees (layers included), handed unchanged to the C-ABI and to the fp64 oracle
(tests/fullwave_pml_oracle.py).  Every source lies on an interior voxel.  Oracle results are computed once per case and shared."""
import functools

import numpy as np

import fullwave_cases as fc
import fullwave_lockin_oracle as lo
import fullwave_oracle as fo
import fullwave_pml_oracle as po


def _cases():
    out = {}
    # the sponge table's own inputs where their sources are interior: uniform water 32^3; the layered medium with its inclusion on the odd
    # anisotropic grid (the medium varies inside the layers, a trace voxel in the corner where three layers overlap); absorption only; density only
    for name in ("uniform_water", "layered", "absorbing_only", "density_only"):
        out[name] = fc.CASES[name]
    n, h = (37, 29, 43), (0.4e-3, 0.5e-3, 0.3e-3)
    pos = [(12.4, 9.7, 8.2), (12.6, 9.2, 8.9), (24.0, 18.0, 8.0), (8.3, 20.1, 7.7)]
    A, tau = [1.0, 0.8, 0.6, 0.9], [0.3, 11.7, 25.2, 40.8]
    # layers of one voxel: r = s_low = exp(-sigma(1) dt / 2) on a single shell, the face depth 1/2 inside it
    out["one_voxel_layers"] = fc._case(n, h, fc.layered(n), 1, pos, A, tau, 300, cycles=2.5, trace=[(18, 14, 30), (0, 0, 0), (36, 28, 42), (0, 14, 20)])
    # an axis with exactly one interior voxel: the sources on it, both of its neighbours layer voxels
    n1 = (13, 21, 23)
    out["one_interior_voxel"] = fc._case(n1, (0.5e-3, 0.4e-3, 0.3e-3), fc.layered(n1), 6, [(6, 10.4, 11.5), (6, 8.0, 9.0)], [1.0, 0.7], [0.2, 5.6], 250,
                                         trace=[(6, 10, 12), (0, 0, 0), (12, 20, 22), (3, 10, 11)])
    # no layers: the two models are the same arithmetic
    out["no_layers"] = fc.CASES["lossless"]
    return out


CASES = _cases()
PARITY = ("uniform_water", "layered", "absorbing_only", "density_only", "one_voxel_layers", "one_interior_voxel")


def _simulate(k, trace):
    return po.simulate(k["n"], k["h"], k["c"], k["rho"], k["alpha"], k["c_ref"], k["pml"], k["pml_alpha"], k["dt"], k["steps"], k["ijk"], k["amp"],
                       k["tau"], k["freq"], k["cycles"], k["ramp"], trace_ijk=trace)


@functools.lru_cache(maxsize=None)
def reference(name):
    ref = _simulate(CASES[name], CASES[name]["trace"])
    for v in ref.values():
        v.setflags(write=False)
    return ref


def _short():
    """a run that ends before anything reaches a layer, or the last interior voxel of an axis (whose + face lies half a voxel inside a layer): 3 steps
    from the middle of the layered grid.  Under the two layer models it is the same run, bit for bit."""
    n, h = (37, 29, 43), (0.4e-3, 0.5e-3, 0.3e-3)
    return fc._case(n, h, fc.layered(n), 6, [(18, 14, 21), (18.4, 14.3, 20.6)], [1.0, 0.7], [0.2, 0.3], 3, trace=[(18, 14, 21), (20, 14, 21), (0, 0, 0)])


SHORT = _short()


def run_device(ctx, name, model="pml", split=None, psq=True):
    """The case through the C-ABI under the layer model -> (p_max, p_min, psq, trace [steps, P])."""
    k = SHORT if name == "short" else CASES[name]
    ctx.fullwave_plan(k["h"], k["n"], k["c"], k["rho"], k["alpha"], k["c_ref"], k["pml"], k["pml_alpha"], k["dt"], layer_model=model)
    ctx.fullwave_sources(fc.lin(k["ijk"], k["n"]), k["amp"], k["tau"], k["freq"], k["cycles"], k["ramp"], k["steps"], points=fc.lin(k["trace"], k["n"]))
    if split is None:
        ctx.fullwave_run(0, k["steps"], psq=psq)
    else:
        ctx.fullwave_run(0, split, psq=psq)
        ctx.fullwave_run(split, k["steps"] - split, psq=psq)
    return ctx.fullwave_fetch()


# ---- lock-in: the volume, and receivers placed inside the layers ----------------------------------------------------------------------
LOCK_CASE = "uniform_water"


def lock_window():
    steps = CASES[LOCK_CASE]["steps"]
    return steps - steps // 3, steps // 3


def lock_table():
    """receivers in voxel units: in the low x layer, in the corner where three layers overlap, across the interior / layer boundary, interior"""
    k = CASES[LOCK_CASE]
    pts = np.array([(2.3, 15.5, 16.25), (1.5, 2.5, 29.75), (5.5, 16.0, 16.0), (16.0, 16.0, 20.0), (30.6, 29.2, 3.3)])
    row, ijk, wt = lo.trilinear(pts * np.asarray(k["h"]), (0, 0, 0), k["h"], k["n"])
    return row.astype(np.int32), fc.lin(ijk, k["n"]), wt


@functools.lru_cache(maxsize=None)
def lock_reference():
    """(C [n], S [n], C_r, S_r) of the oracle"""
    k = CASES[LOCK_CASE]
    every = np.stack(np.meshgrid(*[np.arange(v) for v in k["n"]], indexing="ij"), axis=-1).reshape(-1, 3)
    tr = _simulate(k, every)["trace"]
    w = lock_window()
    C, S = lo.volume_sums(tr, k["freq"], k["dt"], *w)
    row, vox, wt = lock_table()
    Cr, Sr = lo.receiver_sums(tr, {int(v): int(v) for v in vox}, row, vox, wt, k["freq"], k["dt"], *w)
    return C.reshape(k["n"]), S.reshape(k["n"]), Cr, Sr


def run_device_lockin(ctx, model="pml"):
    k = CASES[LOCK_CASE]
    ctx.fullwave_plan(k["h"], k["n"], k["c"], k["rho"], k["alpha"], k["c_ref"], k["pml"], k["pml_alpha"], k["dt"], layer_model=model)
    ctx.fullwave_sources(fc.lin(k["ijk"], k["n"]), k["amp"], k["tau"], k["freq"], k["cycles"], k["ramp"], k["steps"], points=fc.lin(k["trace"], k["n"]))
    row, vox, wt = lock_table()
    w = lock_window()
    ctx.fullwave_lockin(k["freq"], w[0], w[1], volume=True, row=row, voxels=vox, weights=wt)
    ctx.fullwave_run(0, k["steps"], psq=True)
    return ctx.fullwave_fetch(), ctx.fullwave_fetch_lockin()


# ---- element-factored sources: the layered case's elements as (voxel, element, amplitude) entries and per-element (A, tau) ------------
ELEM_CASE = "layered"
ELEM_POS = [(12.4, 9.7, 8.2), (12.6, 9.2, 8.9), (24.0, 18.0, 8.0), (20.5, 12.5, 9.5), (8.3, 20.1, 7.7)]
ELEM_A = [1.0, 0.8, 0.6, 0.0, 0.9]
ELEM_TAU = [0.3, 11.7, 25.2, 3.3, 40.8]


def element_table():
    """(voxels, elements, amplitude per unit A, A [E], tau [E] s): fullwave_cases' "layered" sources with the element's A and delay factored out"""
    k = CASES[ELEM_CASE]
    hh = np.asarray(k["h"])
    vox, el, amp = [], [], []
    for e, p in enumerate(ELEM_POS):
        ijk, a, _ = fo.monopole_entries(np.asarray([p]) * hh, (0, 0, 0), hh, [1.0], [0.0], k["c"], k["freq"], k["dt"], k["n"])
        vox.append(fc.lin(ijk, k["n"])); el.append(np.full(len(a), e, dtype=np.int32)); amp.append(a)
    return np.concatenate(vox), np.concatenate(el), np.concatenate(amp), np.asarray(ELEM_A), np.asarray(ELEM_TAU) * k["dt"]


def run_device_elements(ctx, model="pml"):
    k = CASES[ELEM_CASE]
    vox, el, amp, A, tau = element_table()
    ctx.fullwave_plan(k["h"], k["n"], k["c"], k["rho"], k["alpha"], k["c_ref"], k["pml"], k["pml_alpha"], k["dt"], layer_model=model)
    ctx.fullwave_sources_elements(vox, el, amp, 0.5 * A, tau + 3 * k["dt"], k["freq"], k["cycles"], k["ramp"], k["steps"], points=fc.lin(k["trace"], k["n"]))
    ctx.fullwave_drive(A, tau)          # the drive the reference was made with replaces the first one
    ctx.fullwave_run(0, k["steps"], psq=True)
    return ctx.fullwave_fetch()
