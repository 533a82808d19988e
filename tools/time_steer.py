"""Time the steering-map kernel (kernel 4, steer_map_k) against kernel 2a on the same shape: 256-element 16 x 16 array (3 mm pitch),
256^3 voxels at 0.25 mm from z = 5 mm, 400 kHz.  HIP events on the context's stream, median of `--iters` launches (default 5), the two
kernels in alternating rounds.  Kernel 2a (field_accum_k, pinned with OLX_FIELD_VARIANT=general) runs the same (voxel, element) pair
loop with sin / cos instead of the angle rule.  Prints one line per form of kernel 4 and the ratio to kernel 2a.

`--medium`: the skull-slab leg instead -- the same array, 128^3 voxels at 0.5 mm, a slab of 12 .. 16 planes (c = 2800 m/s, 8 dB/cm/MHz^0.9,
thickness and values varying with x and y) from plane 20: kernel 4h (steer_map_med_k) in its StraightRay + matched and its Direct form,
beside kernel 4 on the same grid and ONE kernel 2h launch (sampled model, one focus) of the same grid and medium."""
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


def skull_slab(shape):
    I, J, K = np.meshgrid(*(np.arange(m) for m in shape), indexing="ij")
    slab = (K >= 20 + (I // 8 + J // 8) % 3) & (K <= 35 - (I // 16) % 2)
    ss = np.full(shape, C, dtype=np.float32)
    att = np.zeros(shape, dtype=np.float32)
    ss[slab] = (2800.0 * (1 + 0.04 * np.sin(0.09 * I + 0.05 * J)))[slab]
    att[slab] = (8.0 * (1 + 0.2 * np.cos(0.06 * I - 0.04 * J)))[slab]
    return ss, att


def medium_leg(ctx, iters, rounds, n=128, h=0.5e-3):
    os.environ.pop("OLX_FIELD_VARIANT", None)
    origin, spacing, shape = (-(n - 1) / 2 * h, -(n - 1) / 2 * h, 5e-3), (h, h, h), (n, n, n)
    ss, att = skull_slab(shape)
    ctx.bf_set_medium(ss, origin, spacing, shape, C)
    ctx.bf_set_attenuation(att, origin, spacing, shape, F0)
    ctx.bf_solve_compensated(np.array([[0.0, 0.0, 45e-3]]), C, mode="matched", use_delay_medium=True)
    ctx.field_plan(origin, spacing, shape, F0, C, RHO, P0, flags=nat.OUT_PMAG)
    ctx.field_set_medium(ss, att, None, model="sampled")
    variant = ctx.field_variant()
    forms = (("4h StraightRay + matched (maxangle 30)", dict(apod_kind=nat.APOD_MAXANGLE, p0=30.0, comp="matched", delays="straight_ray")),
             ("4h Direct (maxangle 30)", dict(apod_kind=nat.APOD_MAXANGLE, p0=30.0, delays="direct")),
             ("4h Direct + matched + spreading + directivity (piecewise 40/20)",
              dict(apod_kind=nat.APOD_PIECEWISE, p0=40.0, p1=20.0, comp="matched", spreading=True, delays="direct", directivity=True)))
    t2h, t4, tm = [], [], {name: [] for name, _ in forms}
    for _ in range(rounds):
        t2h.append(float(np.median(ctx.field_time(iters))))
        ctx.steer_map(origin, spacing, shape, F0, C, P0, apod_kind=nat.APOD_MAXANGLE, p0=30.0)
        t4.append(float(np.median(ctx.steer_time(iters))))
        for name, kw in forms:
            ctx.steer_map_medium(origin, spacing, shape, F0, C, P0, sound_speed=ss, attenuation=att, **kw)
            tm[name].append(float(np.median(ctx.steer_time(iters))))
    fmt = lambda ts: ", ".join(f"{v:.3f}" for v in ts)  # noqa: E731
    print(f"skull slab, 256 elements x {n}^3 at {h * 1e3:g} mm, {int((att != 0).any(axis=(0, 1)).sum())} non-trivial planes", flush=True)
    print(f"kernel 2h ({variant}), one focus: {np.median(t2h):.3f} ms per launch (rounds: {fmt(t2h)})", flush=True)
    print(f"kernel 4 maxangle 30: {np.median(t4):.3f} ms per launch (rounds: {fmt(t4)})", flush=True)
    for name, ts in tm.items():
        print(f"kernel {name}: {np.median(ts):.3f} ms per launch (rounds: {fmt(ts)}), {np.median(ts) / np.median(t2h):.2f} x kernel 2h, "
              f"{np.median(ts) / np.median(t4):.2f} x kernel 4", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--medium", action="store_true", help="the skull-slab leg: kernel 4h beside kernel 4 and kernel 2h on 128^3 at 0.5 mm")
    ap.add_argument("--n", type=int, default=256, help="grid edge")
    ap.add_argument("--rounds", type=int, default=3, help="alternating rounds of (kernel 2a, every form of kernel 4)")
    args = ap.parse_args()
    pos, size, _ = bo.gen_matrix_array(16, 16, 3.0, 0.3)
    ctx = nat.Context(0)
    ctx.set_elements(pos * 1e-3, np.tile([0.0, 0.0, 1.0], (256, 1)), size[:, 0] * size[:, 1] * 1e-6)
    ctx.set_element_apertures(np.tile([1.0, 0.0, 0.0], (256, 1)), size * 1e-3)
    if args.medium:
        return medium_leg(ctx, args.iters, args.rounds)
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
