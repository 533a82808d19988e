#!/usr/bin/env python3
"""Time kernel 6 (eikonal travel times, k_eikonal.hip): ms per solve, sweeps, ms per sweep and achieved bytes/s, for a uniform medium
(no volume streamed), for the bench's skull slab and for a volume filled with the uniform speed (the uniform solve's sweeps and values with
the volume's upload and stream: the difference to "uniform" is what a volume costs).

  python tools/time_eikonal.py [--n 256] [--medium uniform|skull|filled|all] [--repeat 5] [--init-radius 3] [--out profiles/eikonal_time.json]

A solve is one synchronous olx_eikonal_solve (the upload of the sound-speed volume, the init launch, every sweep and the reads of the
sweeps' flags included), timed by the wall clock after one untimed warm-up solve; the median of --repeat solves is reported.  The source
sits off the voxels at (n / 2, n / 2, 0.7 n): an array at the low-z face focusing deep.  Bytes per voxel and sweep are the compulsory
traffic of DESIGN.md section 5.17 -- T read and written once (8 B), plus the sound speed (4 B) with a medium, stencil neighbours served by
the caches -- over the voxels the sweeps were launched over (the init box grown by one voxel per sweep, clipped by the grid).  The achieved
bytes/s are set against the 6.29 TB/s a device-to-device copy reaches on this part."""
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
BYTES = {"uniform": 8, "skull": 12, "filled": 12}


def launched_voxels(n, q, radius, sweeps):
    """Voxels the `sweeps` sweeps were launched over"""
    lo = np.maximum(np.ceil(np.asarray(q) - radius), 0).astype(np.int64)
    hi = np.minimum(np.floor(np.asarray(q) + radius), np.asarray(n) - 1).astype(np.int64)
    total = 0
    for s in range(1, sweeps + 1):
        total += int(np.prod(np.minimum(hi + s, np.asarray(n) - 1) - np.maximum(lo - s, 0) + 1))
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--medium", choices=("uniform", "skull", "filled", "all"), default="all")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--init-radius", type=float, default=3.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, h = a.n, 0.25e-3
    shape = (n, n, n)
    ax = (np.arange(n) - n // 2) * h
    zs = np.arange(n) * h
    q = np.array([n / 2 + 0.3, n / 2 - 0.45, 0.7 * n + 0.2])
    origin = np.array([ax[0], ax[0], zs[0]])
    src = origin + q * h
    media = {}
    if a.medium in ("uniform", "all"):
        media["uniform"] = 1500.0
    if a.medium in ("skull", "all"):
        media["skull"] = np.where(skull_slab_image(ax, ax, zs) > 0, 2800.0, 1500.0).astype(np.float32)
    if a.medium in ("filled", "all"):
        media["filled"] = np.full(shape, 1500.0, dtype=np.float32)
    ctx = nat.Context(0)
    rows = []
    for name, c in media.items():
        ctx.eikonal_solve(origin, (h,) * 3, shape, c, src, init_radius=a.init_radius)
        ms = []
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            sweeps = ctx.eikonal_solve(origin, (h,) * 3, shape, c, src, init_radius=a.init_radius)
            ms.append((time.perf_counter() - t0) * 1e3)
        med = float(np.median(ms))
        tbps = BYTES[name] * launched_voxels(shape, q, a.init_radius, sweeps) / (med * 1e-3) / 1e12
        rows.append({"medium": name, "grid": list(shape), "sweeps": sweeps, "ms_per_solve": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
                     "ms_per_sweep": round(med / sweeps, 5), "bytes_per_voxel_sweep": BYTES[name], "achieved_TBps": round(tbps, 3),
                     "fraction_of_copy": round(tbps / COPY_TBPS, 3)})
        print(json.dumps(rows[-1]), flush=True)
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/time_eikonal.py", "copy_TBps": COPY_TBPS, "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
