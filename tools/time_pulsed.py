"""Launch the pulsed field kernel (2p, field_pulse_k) on the shapes DESIGN.md section 5 reports, for a
`rocprofv3 --kernel-trace --stats -- python tools/time_pulsed.py` run: 256-element 16 x 16 array (3 mm pitch), 20 cycles at
400 kHz, default dt / t_end (pulse_time_axis), 0.25 mm grids of 128^3 and 256^3 with one focus, and 256^3 with the 8 foci
of one shard.  Prints the per-launch time of each shape from HIP events (median of `--iters`)."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "openlifu-python_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from openlifu_amd import _native as nat  # noqa: E402
from openlifu_amd.engine import pulse_time_axis  # noqa: E402
from oracle import bf_oracle as bo  # noqa: E402

F0, C, RHO, P0 = 400e3, 1500.0, 1000.0, 1e5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--only", type=int, default=0, help="one shape only: the single-focus grid of this edge (counter runs)")
    args = ap.parse_args()
    pos, size, _ = bo.gen_matrix_array(16, 16, 3.0, 0.3)
    pos_m = pos * 1e-3
    ctx = nat.Context(0)
    ctx.set_elements(pos_m, np.tile([0.0, 0.0, 1.0], (256, 1)), size[:, 0] * size[:, 1] * 1e-6)
    for n, nfoci in ((args.only, 1),) if args.only else ((128, 1), (256, 1), (256, 8)):
        foci = bo.wheel_targets([0, 0, 35.0], True, nfoci - 1, 5.0)[:nfoci] * 1e-3 if nfoci > 1 else np.array([[0, 0, 35e-3]])
        ctx.bf_solve(foci, C)
        h = 0.25e-3
        origin = (-(n - 1) / 2 * h, -(n - 1) / 2 * h, 5e-3)
        dt, n_t = pulse_time_axis([h] * 3, (n, n, n))
        ctx.field_pulse(20, dt, n_t)
        ctx.field_plan(origin, (h, h, h), (n, n, n), F0, C, RHO, P0, flags=nat.OUT_PMAG | nat.OUT_INTENSITY | nat.OUT_PMAX)
        ms = ctx.field_time(args.iters)
        print(f"{n}^3 x {nfoci} foci: {np.median(ms):.2f} ms per launch ({np.median(ms) / nfoci:.2f} ms per focus), n_t = {n_t}, "
              f"{ctx.field_variant()}", flush=True)
    ctx.field_pulse(0.0, 0.0, 0)
    ctx.sync()


if __name__ == "__main__":
    main()
