#!/usr/bin/env python3
"""Time kernel 5 (full-wave model, k_fullwave.hip): ms per step and achieved bytes/s at 256^3 plus absorbing layers, for the uniform
instantiation and for a skull-slab medium (five coefficient volumes streamed).

  python tools/time_fullwave.py [--n 256] [--pml 16] [--steps 300] [--lockin] [--out profiles/fullwave_time.json]

A run of --steps steps is bracketed by olx_sync (after one untimed warm-up run of 20 steps); the step is three launches (inject,
velocity, pressure-and-record).  Bytes per voxel and step are the compulsory traffic of DESIGN.md section 5.14 -- every volume a launch
reads or writes counted once, stencil neighbours served by the caches: 64 B uniform, 84 B with a medium, + 8 B with sum p^2.  The
achieved bytes/s are set against the 6.29 TB/s a device-to-device copy reaches on this part.

--lockin adds, per medium, runs whose lock-in window is the whole run: the volume sums (+ 16 B per voxel and
step: C and S read and written), and the volume sums with 64 receivers of 8 entries each (one more launch of one block per step)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--pml", type=int, default=16)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--lockin", action="store_true", help="also time the steps inside a lock-in window")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
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
        ctx.fullwave_plan((h,) * 3, shape, c, rho, alpha, 1500.0, a.pml, 2.0, dt)
        ctx.fullwave_sources(src, [1.0], [0.0], 500e3, 1e6, 0.0, a.steps)
        for psq in (False, True):
            ctx.fullwave_run(0, 20, psq=psq)
            ctx.sync()
            t0 = time.perf_counter()
            ctx.fullwave_run(0, a.steps, psq=psq)
            ctx.sync()
            ms = (time.perf_counter() - t0) * 1e3 / a.steps
            b = BYTES[name] + (8 if psq else 0)
            tbps = b * vox / (ms * 1e-3) / 1e12
            rows.append({"medium": name, "sum_p2": psq, "grid": list(shape), "steps": a.steps, "ms_per_step": round(ms, 4), "bytes_per_voxel_step": b,
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
            b = BYTES[name] + 16
            tbps = b * vox / (ms * 1e-3) / 1e12
            rows.append({"medium": name, "sum_p2": False, "lockin": label, "grid": list(shape), "steps": a.steps, "ms_per_step": round(ms, 4),
                         "bytes_per_voxel_step": b, "achieved_TBps": round(tbps, 3), "fraction_of_copy": round(tbps / COPY_TBPS, 3)})
            print(json.dumps(rows[-1]), flush=True)
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/time_fullwave.py", "copy_TBps": COPY_TBPS, "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
