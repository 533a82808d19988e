#!/usr/bin/env python3
"""Time kernel 5 (full-wave model, k_fullwave.hip): ms per step and achieved bytes/s at 256^3 plus absorbing layers, for the uniform
instantiation and for a skull-slab medium (five coefficient volumes streamed).

  python tools/time_fullwave.py [--n 256] [--pml 16] [--steps 300] [--layers pml] [--lockin | --aperture [--rounds 3] | --response M [--rounds 3]] [--out profiles/fullwave_time.json]

A run of --steps steps is bracketed by olx_sync (after one untimed warm-up run of 20 steps); the step is three launches (inject,
velocity, pressure-and-record).  Bytes per voxel and step are the compulsory traffic of DESIGN.md section 5.14 -- every volume a launch
reads or writes counted once, stencil neighbours served by the caches: 64 B uniform, 84 B with a medium, + 8 B with sum p^2.  The
achieved bytes/s are set against the 6.29 TB/s a device-to-device copy reaches on this part.

--lockin adds, per medium, runs whose lock-in window is the whole run: the volume sums (+ 16 B per voxel and
step: C and S read and written), and the volume sums with 64 receivers of 8 entries each (one more launch of one block per step).

--aperture times the element-factored sources of DESIGN.md section 5.18 instead: a 16 x 16 array of 2.9 mm elements (pitch 3 mm) at
upsampling rate 5 on the uniform medium, against the same array as 256 point sources -- the two alternate in ONE process on ONE box
(--rounds times each, the median is reported) -- with the number of (element, voxel) entries, and the build of the weight table on the
device (olx_fullwave_apertures, wall time of the call) against a NumPy scatter build of the same table (np.add.at over the 8 corners
of every point).

--response M times the fill of the drive table through drive taps next to the run itself: 256 point elements in
element-factored form, one class of M Hann-windowed taps at the drive frequency on all of them, --steps steps.  olx_fullwave_drive re-fills the
table -- two small uploads (A, tau) and the launches, fullwave_drive_k alone for the bare drive, fullwave_drive_k over the extended range plus
fullwave_drive_fir_k with the response -- between two olx_sync; the median of --rounds calls of each is reported, with the run's ms per step.
The figure is the wall time of the whole call (host checks, a stream synchronise, the two uploads, the launches, the final sync): an upper
bound on the launches, of which the bare fill shows the share that is not the response's ("response_minus_bare_ms").  The figures of DESIGN.md
section 5.20 are `--response 64 --steps 4000 --rounds 5` and `--response 256 --steps 4000 --rounds 5`."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "openlifu-python_amd"), ROOT]

from openlifu_amd import _native as nat  # noqa: E402
from openlifu_amd.seg.seg_methods.threshold import skull_slab_image  # noqa: E402

COPY_TBPS = 6.29
BYTES = {"uniform": 64, "medium": 84}


def numpy_scatter_table(centre, size, nw, nl, h, n):
    """The aperture weights of axis-aligned elements by a NumPy scatter: every point on its 8 corners, merged per (element, voxel)"""
    row, vox, wt = [0], [], []
    for e in range(len(centre)):
        sa = np.repeat((np.arange(nw[e]) + 0.5) / nw[e] - 0.5, nl[e])
        sb = np.tile((np.arange(nl[e]) + 0.5) / nl[e] - 0.5, nw[e])
        q = (centre[e] + np.stack([sa * size[e, 0], sb * size[e, 1], np.zeros_like(sa)], axis=1)) / h
        near = np.rint(q)
        q = np.where(np.abs(q - near) <= 1e-9, near, q)
        lo = np.floor(q).astype(np.int64)
        f = q - lo
        keys, vals = [], []
        for di in (0, 1):
            for dj in (0, 1):
                for dk in (0, 1):
                    w = (f[:, 0] if di else 1 - f[:, 0]) * (f[:, 1] if dj else 1 - f[:, 1]) * (f[:, 2] if dk else 1 - f[:, 2])
                    keys.append(((lo[:, 0] + di) * n + lo[:, 1] + dj) * n + lo[:, 2] + dk); vals.append(w)
        keys, vals = np.concatenate(keys), np.concatenate(vals)
        uniq, inv = np.unique(keys, return_inverse=True)
        sums = np.zeros(uniq.size)
        np.add.at(sums, inv, vals)
        keep = sums != 0
        vox.append(uniq[keep]); wt.append(sums[keep] / (nw[e] * nl[e])); row.append(row[-1] + int(keep.sum()))
    return np.asarray(row), np.concatenate(vox), np.concatenate(wt)


def aperture_main(a):
    n = a.n + 2 * a.pml
    h = 0.25e-3
    shape = (n, n, n)
    dt = 0.9 * 6.0 / (7.0 * 1500.0 * np.sqrt(3.0) / h)
    g = (np.arange(16) - 7.5) * 3.0e-3 + (n // 2 + 0.3) * h
    centre = np.array([[x, y, (a.pml + 2.3) * h] for x in g for y in g])
    E = len(centre)
    size = np.full((E, 2), 2.9e-3)
    nw = nl = np.full(E, int(np.ceil(5 * 2.9e-3 / h - 1e-9)), dtype=np.int32)
    u, v = np.tile([1.0, 0.0, 0.0], (E, 1)), np.tile([0.0, 1.0, 0.0], (E, 1))
    A, tau = np.ones(E), (np.arange(E) % 7) * 0.37 * dt
    ctx = nat.Context(0)
    ctx.fullwave_plan((h,) * 3, shape, 1500.0, 1000.0, 0.0, 1500.0, a.pml, 2.0, dt)
    ctx.fullwave_apertures(centre, u, v, size, nw, nl)          # (untimed: the first call creates the buffers)
    t0 = time.perf_counter()
    row, vox, wt = ctx.fullwave_apertures(centre, u, v, size, nw, nl)
    t_dev = time.perf_counter() - t0
    t0 = time.perf_counter()
    r2, v2, w2 = numpy_scatter_table(centre, size, nw, nl, h, n)
    t_np = time.perf_counter() - t0
    assert np.array_equal(row, r2) and np.array_equal(vox, v2) and np.abs(wt - w2).max() <= 1e-12
    el = np.repeat(np.arange(E, dtype=np.int32), np.diff(row))
    scale = dt * 1500.0 ** 2 * 4 * np.pi / (2 * np.pi * 500e3 * h ** 3)
    # the same array as point sources: one trilinear monopole per element (8 entries each)
    pr, pv, pw = numpy_scatter_table(centre, np.zeros((E, 2)), np.ones(E, dtype=np.int32), np.ones(E, dtype=np.int32), h, n)
    pe = np.repeat(np.arange(E), np.diff(pr))

    def point():
        ctx.fullwave_sources(pv, pw * scale * A[pe], tau[pe], 500e3, 1e6, 0.0, a.steps)

    def aperture():
        ctx.fullwave_sources_elements(vox, el, wt * scale, A, tau, 500e3, 1e6, 0.0, a.steps)

    times = {"point": [], "aperture": []}
    for _ in range(a.rounds):
        for name, set_sources in (("point", point), ("aperture", aperture)):
            set_sources()
            ctx.fullwave_run(0, 20)
            ctx.sync()
            t0 = time.perf_counter()
            ctx.fullwave_run(0, a.steps)
            ctx.sync()
            times[name].append((time.perf_counter() - t0) * 1e3 / a.steps)
    ctx.close()
    out = {"tool": "tools/time_fullwave.py --aperture", "grid": list(shape), "steps": a.steps, "rounds": a.rounds, "elements": E,
           "points_per_element": int(nw[0]) * int(nl[0]), "entries": {"point": int(pv.size), "aperture": int(vox.size)},
           "ms_per_step": {k: round(float(np.median(t)), 4) for k, t in times.items()}, "ms_per_step_all": {k: [round(x, 4) for x in t] for k, t in times.items()},
           "aperture_over_point": round(float(np.median(times["aperture"]) / np.median(times["point"])), 4),
           "table_build_ms": {"device": round(t_dev * 1e3, 3), "numpy_scatter": round(t_np * 1e3, 3)}}
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


def response_main(a):
    n = a.n + 2 * a.pml
    h = 0.25e-3
    shape = (n, n, n)
    dt = 0.9 * 6.0 / (7.0 * 1500.0 * np.sqrt(3.0) / h)
    g = (np.arange(16) - 7.5) * 3.0e-3 + (n // 2 + 0.3) * h
    centre = np.array([[x, y, (a.pml + 2.3) * h] for x in g for y in g])
    E, M = len(centre), a.response
    A, tau = np.ones(E), (np.arange(E) % 7) * 0.37 * dt
    scale = dt * 1500.0 ** 2 * 4 * np.pi / (2 * np.pi * 500e3 * h ** 3)
    pr, pv, pw = numpy_scatter_table(centre, np.zeros((E, 2)), np.ones(E, dtype=np.int32), np.ones(E, dtype=np.int32), h, n)
    pe = np.repeat(np.arange(E, dtype=np.int32), np.diff(pr))
    m = np.arange(M, dtype=np.float64)
    taps = 0.5 * (1.0 - np.cos(2.0 * np.pi * (m + 1.0) / (M + 1.0))) * np.cos(2.0 * np.pi * 500e3 * dt * m)
    ctx = nat.Context(0)
    ctx.fullwave_plan((h,) * 3, shape, 1500.0, 1000.0, 0.0, 1500.0, a.pml, 2.0, dt)
    ctx.fullwave_sources_elements(pv, pe, pw * scale, A, tau, 500e3, 1e6, 0.0, a.steps)
    fills = {"bare": [], "response": []}
    for name in ("bare", "response"):
        if name == "response":
            ctx.fullwave_drive_response(np.zeros(E, dtype=np.int32), [taps])          # (untimed: the first call creates the buffers)
        ctx.fullwave_drive(A, tau)
        ctx.sync()
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            ctx.fullwave_drive(A, tau)
            ctx.sync()
            fills[name].append((time.perf_counter() - t0) * 1e3)
    ctx.fullwave_run(0, 20)
    ctx.sync()
    t0 = time.perf_counter()
    ctx.fullwave_run(0, a.steps)
    ctx.sync()
    run_ms = (time.perf_counter() - t0) * 1e3
    ctx.close()
    fill = float(np.median(fills["response"]))
    out = {"tool": "tools/time_fullwave.py --response", "grid": list(shape), "steps": a.steps, "rounds": a.rounds, "elements": E, "taps": M,
           "fill_ms": {k: round(float(np.median(t)), 4) for k, t in fills.items()}, "fill_ms_all": {k: [round(x, 4) for x in t] for k, t in fills.items()},
           "response_minus_bare_ms": round(fill - float(np.median(fills["bare"])), 4),
           "run_ms": round(run_ms, 2), "ms_per_step": round(run_ms / a.steps, 4), "fill_over_run": round(fill / run_ms, 6)}
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--pml", type=int, default=16)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--lockin", action="store_true", help="also time the steps inside a lock-in window")
    ap.add_argument("--out", default=None)
    ap.add_argument("--aperture", action="store_true", help="time 256 aperture elements against 256 point sources (section 5.18)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers", choices=("sponge", "pml"), default="sponge", help="the layer model (section 5.19): pml = split layers")
    ap.add_argument("--response", type=int, default=0, metavar="M", help="time the drive-table fill through M taps next to the run (section 5.20)")
    a = ap.parse_args()
    if a.aperture:
        return aperture_main(a)
    if a.response:
        if not 1 <= a.response <= 256:
            ap.error("--response takes 1 .. 256 taps")
        return response_main(a)
    layer_bytes = 24.0 * (1.0 - (a.n / (a.n + 2.0 * a.pml)) ** 3) if a.layers == "pml" else 0.0      # three components read and written in the layer voxels
    n = a.n + 2 * a.pml
    h = 0.25e-3
    shape = (n, n, n)
    ax = (np.arange(n) - n // 2) * h
    bone = skull_slab_image(ax, ax, (np.arange(n) - a.pml) * h) > 0
    media = {"uniform": (1500.0, 1000.0, 0.0),
             "medium": (np.where(bone, 2800.0, 1500.0).astype(np.float32), np.where(bone, 1900.0, 1000.0).astype(np.float32),
                        np.where(bone, 37.0, 0.0).astype(np.float32))}
    ctx = nat.Context(0)
    vox = n ** 3
    src = [(n // 2 * n + n // 2) * n + a.pml + 2]
    rows = []
    for name, (c, rho, alpha) in media.items():
        dt = 0.9 * 6.0 / (7.0 * float(np.max(c)) * np.sqrt(3.0) / h)
        ctx.fullwave_plan((h,) * 3, shape, c, rho, alpha, 1500.0, a.pml, 2.0, dt, layer_model=a.layers)
        ctx.fullwave_sources(src, [1.0], [0.0], 500e3, 1e6, 0.0, a.steps)
        for psq in (False, True):
            ctx.fullwave_run(0, 20, psq=psq)
            ctx.sync()
            t0 = time.perf_counter()
            ctx.fullwave_run(0, a.steps, psq=psq)
            ctx.sync()
            ms = (time.perf_counter() - t0) * 1e3 / a.steps
            b = round(BYTES[name] + (8 if psq else 0) + layer_bytes, 2)
            tbps = b * vox / (ms * 1e-3) / 1e12
            rows.append({"medium": name, "layers": a.layers, "sum_p2": psq, "grid": list(shape), "steps": a.steps, "ms_per_step": round(ms, 4), "bytes_per_voxel_step": b,
                         "achieved_TBps": round(tbps, 3), "fraction_of_copy": round(tbps / COPY_TBPS, 3)})
            print(json.dumps(rows[-1]), flush=True)
        if not a.lockin:
            continue
        rng = np.random.default_rng(0)
        table = dict(row=np.arange(65) * 8, voxels=rng.integers(0, vox, 64 * 8), weights=np.full(64 * 8, 0.125))
        for label, kw in (("volume", {}), ("volume + 64 receivers", table)):
            ctx.fullwave_lockin(500e3, 0, a.steps, volume=True, **kw)
            ctx.fullwave_run(0, 20)
            ctx.sync()
            t0 = time.perf_counter()
            ctx.fullwave_run(0, a.steps)
            ctx.sync()
            ms = (time.perf_counter() - t0) * 1e3 / a.steps
            b = round(BYTES[name] + 16 + layer_bytes, 2)
            tbps = b * vox / (ms * 1e-3) / 1e12
            rows.append({"medium": name, "layers": a.layers, "sum_p2": False, "lockin": label, "grid": list(shape), "steps": a.steps, "ms_per_step": round(ms, 4),
                         "bytes_per_voxel_step": b, "achieved_TBps": round(tbps, 3), "fraction_of_copy": round(tbps / COPY_TBPS, 3)})
            print(json.dumps(rows[-1]), flush=True)
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/time_fullwave.py", "copy_TBps": COPY_TBPS, "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
