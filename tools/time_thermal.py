"""Time the thermal model's step kernel (kernel 3, thermal_step_k) on the shapes DESIGN.md section 5.8 reports, for a
`rocprofv3 --kernel-trace --stats -- python tools/time_thermal.py` run: 0.25 mm grids of 128^3 and 256^3, uniform water and the
C5 skull slab of SURVEY section 8(d) (water / skull, the example protocol's materials), one focus, one 20 us pulse every 100 ms.
Prints ms per step (host clock around `--steps` steps ending in a device synchronise, after a warm-up), the algorithmic bytes
per step and their rate as a fraction of the 8 TB/s HBM peak.  Bytes per voxel and step: dT read + write (8), rise_max read +
write (8), CEM43 read + write (8), and for a heterogeneous medium the coefficients (float4, 16) and 1 / (rho Cp) (4); a step with
a pulse adds s(v) (heterogeneous only, 4) and 4 per active focus -- neighbour reads are counted once (cache reuse)."""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "openlifu-python_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from openlifu_amd import _native as nat  # noqa: E402
from openlifu_amd.seg.seg_methods.threshold import skull_slab_image  # noqa: E402
from openlifu_amd.sim import thermal as th  # noqa: E402

PEAK = 8.0e12
WATER = (1000.0, 4182.0, 0.598, 0.0022)
SKULL = (1900.0, 1300.0, 0.4, 6.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    ctx = nat.Context(0)
    h = 0.25e-3
    f0 = 400e3
    for n in (128, 256):
        xs = (np.arange(n) - (n - 1) / 2) * h
        zs = 5e-3 + np.arange(n) * h
        bone = skull_slab_image(xs, xs, zs) > 0
        inten = np.zeros((1, n, n, n), dtype=np.float32)
        inten[0, n // 2 - 8:n // 2 + 8, n // 2 - 8:n // 2 + 8, :] = 10.0
        for kind in ("uniform", "skull"):
            if kind == "uniform":
                med = [float(v) for v in WATER]
            else:
                med = [np.where(bone, s, w).astype(np.float32) for w, s in zip(WATER, SKULL)]
            alpha = med[3] * th._np_per_m(1.0, f0)
            dt_max = ctx.thermal_plan((0.0, 0.0, 0.0), (h, h, h), (n, n, n), med[0], med[1], med[2], alpha)
            dt = dt_max / 2
            total = args.warmup + args.steps
            pulse_every = max(1, int(round(0.1 / dt)))
            on = (np.arange(total) % pulse_every) == 0
            row_ptr = np.concatenate([[0], np.cumsum(on)]).astype(np.int32)
            ctx.thermal_schedule(row_ptr, np.zeros(int(on.sum()), dtype=np.int32), np.full(int(on.sum()), 2e-5))
            ctx.thermal_source(1, inten)
            ctx.thermal_run(dt, 37.0, 0, args.warmup)
            ctx.sync()
            t0 = time.perf_counter()
            ctx.thermal_run(dt, 37.0, args.warmup, args.steps)
            ctx.sync()
            ms = (time.perf_counter() - t0) * 1e3 / args.steps
            vox = n ** 3
            per_vox = 24 + (20 if kind == "skull" else 0)
            src_steps = int(on[args.warmup:].sum())
            bytes_step = vox * (per_vox + (4 + (4 if kind == "skull" else 0)) * src_steps / args.steps)
            print(f"{n}^3 {kind}: {ms:.4f} ms per step, {bytes_step / 1e6:.1f} MB per step ({per_vox} B/voxel + source), "
                  f"{bytes_step / (ms * 1e-3) / 1e12:.2f} TB/s = {bytes_step / (ms * 1e-3) / PEAK:.1%} of 8 TB/s, dt = {dt * 1e3:.2f} ms, "
                  f"{src_steps} source steps", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
