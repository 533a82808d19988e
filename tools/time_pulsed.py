"""Launch the pulsed field kernel (2p, field_pulse_k) on the shapes DESIGN.md section 5 reports, for a
`rocprofv3 --kernel-trace --stats -- python tools/time_pulsed.py` run: 256-element 16 x 16 array (3 mm pitch), 20 cycles at
400 kHz, default dt / t_end (pulse_time_axis), 0.25 mm grids of 128^3 and 256^3 with one focus, and 256^3 with the 8 foci
of one shard.  Prints the per-launch time of each shape from HIP events (median of `--iters`).  `--pii` plans with OUT_PII (the
<PII> instantiation), `--trace N` also times one olx_field_pulse_trace of N points per shape (host clock around the synchronous call:
table, memset, kernel and the copy out).  `--medium` puts the skull slab of BASELINE configs[4] into the timed grid (skull_slab_volumes; the
water's own 0.0022 dB/cm/MHz dropped, so that only the slab's planes are non-trivial) and times, per shape, kernel 2p (no medium), kernel 2h
(the sampled continuous-wave kernel through the same medium: 2h + 2p per focus is the yardstick) and kernel 2ph (olx_field_pulse_medium).
`--response M` also times each shape with one class of M Hann-windowed taps at the drive frequency (olx_field_pulse_response, the RESP
instantiations) after the plain plan."""
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
from openlifu_amd.engine import pulse_time_axis  # noqa: E402
from openlifu_amd.seg.seg_methods import skull_slab_volumes  # noqa: E402
from oracle import bf_oracle as bo  # noqa: E402

F0, C, RHO, P0 = 400e3, 1500.0, 1000.0, 1e5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--only", type=int, default=0, help="one shape only: the single-focus grid of this edge (counter runs)")
    ap.add_argument("--pii", action="store_true", help="plan with OUT_PII: the pulse intensity integral volume")
    ap.add_argument("--trace", type=int, default=0, help="also time olx_field_pulse_trace of this many points")
    ap.add_argument("--medium", action="store_true", help="skull slab in the grid: time kernels 2p, 2h (sampled) and 2ph per shape")
    ap.add_argument("--response", type=int, default=0, help="also time the plan with a Hann-windowed impulse response of this many taps")
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
        flags = nat.OUT_PMAG | nat.OUT_INTENSITY | nat.OUT_PMAX | (nat.OUT_PII if args.pii else 0)
        if args.medium:
            axes = [origin[a] + np.arange(n) * h for a in range(3)]
            vol = skull_slab_volumes(*axes)
            vol["attenuation"] = np.where(vol["sound_speed"] != np.float32(C), vol["attenuation"], 0.0).astype(np.float32)
            ctx.field_pulse(0.0, 0.0, 0)
            ctx.field_plan(origin, (h, h, h), (n, n, n), F0, C, RHO, P0, flags=nat.OUT_PMAG | nat.OUT_INTENSITY)
            ctx.field_set_medium(vol["sound_speed"], vol["attenuation"], vol["density"], model="sampled")
            ms = ctx.field_time(args.iters)
            print(f"{n}^3 x {nfoci} foci, kernel 2h: {np.median(ms):.2f} ms per launch, {ctx.field_variant()}", flush=True)
        ctx.field_pulse(20, dt, n_t)
        ctx.field_plan(origin, (h, h, h), (n, n, n), F0, C, RHO, P0, flags=flags)
        ms = ctx.field_time(args.iters)
        print(f"{n}^3 x {nfoci} foci{' + PII' if args.pii else ''}: {np.median(ms):.2f} ms per launch ({np.median(ms) / nfoci:.2f} ms per focus), "
              f"n_t = {n_t}, {ctx.field_variant()}", flush=True)
        if args.response:
            m = np.arange(args.response)
            taps = (0.5 - 0.5 * np.cos(2 * np.pi * (m + 0.5) / args.response)) * np.sin(2 * np.pi * F0 * dt * m + 0.3)
            ctx.field_pulse_response(np.zeros(256, dtype=np.int32), [taps])
            ctx.field_plan(origin, (h, h, h), (n, n, n), F0, C, RHO, P0, flags=flags)
            ms_r = ctx.field_time(args.iters)
            print(f"{n}^3 x {nfoci} foci{' + PII' if args.pii else ''}, {args.response}-tap response: {np.median(ms_r):.2f} ms per launch "
                  f"({np.median(ms_r) / np.median(ms):.2f} x the plain plan), {ctx.field_variant()}", flush=True)
            ctx.field_pulse_response()
            ctx.field_plan(origin, (h, h, h), (n, n, n), F0, C, RHO, P0, flags=flags)      # (what follows times the plain plan)
        if args.medium:
            ctx.field_pulse_medium(vol["sound_speed"], vol["attenuation"], vol["density"])
            ms = ctx.field_time(args.iters)
            print(f"{n}^3 x {nfoci} foci{' + PII' if args.pii else ''} through the slab: {np.median(ms):.2f} ms per launch "
                  f"({np.median(ms) / nfoci:.2f} ms per focus), {ctx.field_variant()}", flush=True)
        if args.trace:
            vox = np.random.default_rng(7).integers(0, n ** 3, size=args.trace)
            ctx.field_pulse_trace(vox)          # (warm-up: code object, buffers)
            ts = []
            for _ in range(max(args.iters, 3)):
                t0 = time.perf_counter()
                ctx.field_pulse_trace(vox)
                ts.append(1e3 * (time.perf_counter() - t0))
            print(f"{n}^3 x {nfoci} foci: trace of {args.trace} points {np.median(ts):.2f} ms per call (host clock, copy out included)", flush=True)
    ctx.field_pulse(0.0, 0.0, 0)
    ctx.sync()


if __name__ == "__main__":
    main()
