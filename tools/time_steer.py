"""Time the steering-map kernel (kernel 4, steer_map_k) against kernel 2a on the same shape: 256-element 16 x 16 array (3 mm pitch),
256^3 voxels at 0.25 mm from z = 5 mm, 400 kHz.  HIP events on the context's stream, median of `--iters` launches (default 5), the two
kernels in alternating rounds.  Kernel 2a (field_accum_k, pinned with OLX_FIELD_VARIANT=general) runs the same (voxel, element) pair
loop with sin / cos instead of the angle rule.  Prints one line per form of kernel 4 and the ratio to kernel 2a."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

os.environ["OLX_FIELD_VARIANT"] = "general"      # kernel 2a for the reference launches (read at plan time)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "openlifu-python_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from openlifu_amd import _native as nat  # noqa: E402
from oracle import bf_oracle as bo  # noqa: E402

F0, C, RHO, P0 = 400e3, 1500.0, 1000.0, 1e5
FORMS = (("uniform", (nat.APOD_UNIFORM, 1.0, 0.0), 0.0, False), ("maxangle 30", (nat.APOD_MAXANGLE, 30.0, 0.0), 0.0, False),
         ("piecewise 40/20", (nat.APOD_PIECEWISE, 40.0, 20.0), 0.0, False), ("uniform + absorption", (nat.APOD_UNIFORM, 1.0, 0.0), 5.0, False),
         ("maxangle 30 + directivity + absorption", (nat.APOD_MAXANGLE, 30.0, 0.0), 5.0, True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--n", type=int, default=256, help="grid edge")
    ap.add_argument("--rounds", type=int, default=3, help="alternating rounds of (kernel 2a, every form of kernel 4)")
    args = ap.parse_args()
    pos, size, _ = bo.gen_matrix_array(16, 16, 3.0, 0.3)
    ctx = nat.Context(0)
    ctx.set_elements(pos * 1e-3, np.tile([0.0, 0.0, 1.0], (256, 1)), size[:, 0] * size[:, 1] * 1e-6)
    ctx.set_element_apertures(np.tile([1.0, 0.0, 0.0], (256, 1)), size * 1e-3)
    n, h = args.n, 0.25e-3
    origin, spacing, shape = (-(n - 1) / 2 * h, -(n - 1) / 2 * h, 5e-3), (h, h, h), (n, n, n)
    ctx.bf_solve(np.array([[0.0, 0.0, 35e-3]]), C)
    ctx.field_plan(origin, spacing, shape, F0, C, RHO, P0, flags=nat.OUT_PMAG | nat.OUT_INTENSITY)
    variant = ctx.field_variant()
    t2a, t4 = [], {name: [] for name, *_ in FORMS}
    for _ in range(args.rounds):
        t2a.append(float(np.median(ctx.field_time(args.iters))))
        for name, (kind, p0, p1), absorption, directivity in FORMS:
            ctx.steer_map(origin, spacing, shape, F0, C, P0, apod_kind=kind, p0=p0, p1=p1, absorption=absorption, directivity=directivity)
            t4[name].append(float(np.median(ctx.steer_time(args.iters))))
    ref = float(np.median(t2a))
    print(f"kernel 2a ({variant}), 256 elements x {n}^3: {ref:.3f} ms per launch (rounds: {', '.join(f'{t:.3f}' for t in t2a)})", flush=True)
    for name, ts in t4.items():
        t = float(np.median(ts))
        print(f"kernel 4 {name}: {t:.3f} ms per launch (rounds: {', '.join(f'{v:.3f}' for v in ts)}), {t / ref:.2f} x kernel 2a, "
              f"{256 * n ** 3 / t * 1e-6:.1f} G pairs/s", flush=True)


if __name__ == "__main__":
    main()
