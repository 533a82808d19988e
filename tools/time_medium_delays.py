"""Time kernel 1m (bf_med_k, StraightRay delays) on BASELINE configs[4]'s case and measure its focal gain against Direct, for a
`rocprofv3 --kernel-trace --stats -- python tools/time_medium_delays.py` run: the 256-element 16 x 16 array (3 mm
pitch), the 256^3 0.25 mm grid of the SURVEY 8(d) skull-slab phantom (SkullThreshold segmentation), 8 foci of a wheel at 40 mm moved to
their nearest voxels.  Prints the host time of olx_bf_set_medium and of each olx_bf_solve_medium (kernel 1 + kernel 1m + the copies), and
|p| at each focus with StraightRay over Direct delays for the sampled (kernel 2h) and the "auto" (marched, kernel 2m) field models.

``--apod`` times kernel 1a the same way instead: olx_bf_set_attenuation, then olx_bf_solve_compensated alone
(bf_med_k<false, true>) and in one walk with the delays (bf_med_k<true, true>) next to olx_bf_solve_medium (bf_med_k<true, false>) in the
same process, and reports what MediumCompensated buys on the case: the spread max / min of the per-element arrival amplitude before and
after "equalize", and |p(focus)| / sqrt(sum apod^2) of "matched" over Uniform for both field models."""
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
from openlifu_amd.seg.seg_methods import skull_slab_volumes  # noqa: E402

C, F0, RHO, P0 = 1500.0, 400e3, 1000.0, 1e5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--no-gain", action="store_true", help="timing only")
    ap.add_argument("--apod", action="store_true", help="time kernel 1a (MediumCompensated) and report what it buys")
    args = ap.parse_args()
    ctx = nat.Context(0)
    n, h = 256, 0.25e-3
    xs = (np.arange(n) - (n - 1) / 2) * h
    zs = 5e-3 + np.arange(n) * h
    origin, spacing = (xs[0], xs[0], zs[0]), (h, h, h)
    vol = skull_slab_volumes(xs, xs, zs)
    a = (np.arange(16) - 7.5) * 3e-3
    pos = np.stack(np.meshgrid(a, a, indexing="ij"), axis=-1).reshape(-1, 2)
    pos = np.column_stack([pos, np.zeros(len(pos))])
    ctx.set_elements(pos, np.tile([0.0, 0.0, 1.0], (len(pos), 1)), np.full(len(pos), 2.7e-3 ** 2))
    ang = np.arange(7) * 2 * np.pi / 7
    wheel = np.vstack([[0, 0, 40e-3], np.column_stack([5e-3 * np.cos(ang), 5e-3 * np.sin(ang), np.full(7, 40e-3)])])
    idx = np.column_stack([np.argmin(np.abs(xs[None] - wheel[:, :1]), axis=1), np.argmin(np.abs(xs[None] - wheel[:, 1:2]), axis=1),
                           np.argmin(np.abs(zs[None] - wheel[:, 2:3]), axis=1)])
    foci = np.column_stack([xs[idx[:, 0]], xs[idx[:, 1]], zs[idx[:, 2]]])
    t0 = time.perf_counter()
    ctx.bf_set_medium(vol["sound_speed"], origin, spacing, (n, n, n), C)
    print(f"olx_bf_set_medium (256^3, host scan + upload of the held planes): {(time.perf_counter() - t0) * 1e3:.1f} ms", flush=True)
    for _ in range(args.warmup):
        ctx.bf_solve_medium(foci, C)
    ts = []
    for _ in range(args.iters):
        t0 = time.perf_counter()
        d_sr, _ = ctx.bf_solve_medium(foci, C)
        ts.append(time.perf_counter() - t0)
    print(f"olx_bf_solve_medium, 8 foci x 256 elements: host {np.median(ts) * 1e6:.1f} us median, {np.mean(ts) * 1e6:.1f} us mean "
          f"over {args.iters} calls (kernel times: the rocprofv3 stats of bf_med_k / bf_solve_k)", flush=True)
    if args.apod:
        return apod(ctx, args, vol, origin, spacing, n, foci, idx, pos)
    if args.no_gain:
        return
    d_d, _ = ctx.bf_solve(foci, C)
    for model in ("sampled", "auto"):
        p = {}
        for name, d in (("straightray", d_sr), ("direct", d_d)):
            ctx.set_steering(d, np.ones_like(d))
            ctx.field_plan(origin, spacing, (n, n, n), F0, C, RHO, P0, flags=nat.OUT_PMAG)
            ctx.field_set_medium(vol["sound_speed"], vol["attenuation"], vol["density"], model=model)
            variant = ctx.field_variant()
            ctx.field_launch()
            p[name] = np.array([ctx.field_fetch(f, want=("pmag",))["pmag"][tuple(idx[f])] for f in range(len(foci))])
        g = p["straightray"] / p["direct"]
        print(f"{model} ({variant}): |p(focus)| StraightRay / Direct = {g.min():.3f} .. {g.max():.3f}, mean {g.mean():.3f}", flush=True)
    ctx.close()


def apod(ctx, args, vol, origin, spacing, n, foci, idx, pos):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import medium_apod_oracle as ao
    t0 = time.perf_counter()
    ctx.bf_set_attenuation(vol["attenuation"], origin, spacing, (n, n, n), F0)
    print(f"olx_bf_set_attenuation (256^3, host scan + upload of the held planes): {(time.perf_counter() - t0) * 1e3:.1f} ms", flush=True)
    for name, kw in (("attenuation only", {}), ("one walk with the delays", {"use_delay_medium": True})):
        for _ in range(args.warmup):
            ctx.bf_solve_compensated(foci, C, mode="matched", **kw)
        ts = []
        for _ in range(args.iters):
            t0 = time.perf_counter()
            ctx.bf_solve_compensated(foci, C, mode="matched", **kw)
            ts.append(time.perf_counter() - t0)
        print(f"olx_bf_solve_compensated ({name}), 8 foci x 256 elements: host {np.median(ts) * 1e6:.1f} us median, {np.mean(ts) * 1e6:.1f} us mean "
              f"over {args.iters} calls", flush=True)
    if args.no_gain:
        return
    area = np.full(len(pos), 2.7e-3 ** 2)
    A, h, d = ao.arrival(pos, foci, vol["attenuation"], origin, spacing, F0, area=area)
    d_sr, a_eq = ctx.bf_solve_compensated(foci, C, mode="equalize", spreading=True, use_delay_medium=True)
    print(f"oracle: A_e {A.min():.3f} .. {A.max():.3f} Np; arrival amplitude max / min per focus: Uniform {(h.max(axis=1) / h.min(axis=1)).max():.4f}, "
          f"equalize + spreading {((a_eq * h).max(axis=1) / (a_eq * h).min(axis=1)).max():.12f}", flush=True)
    _, a_m = ctx.bf_solve_compensated(foci, C, mode="matched", spreading=True, use_delay_medium=True)
    for model in ("sampled", "auto"):
        q = {}
        for name, a in (("uniform", np.ones_like(a_m)), ("matched", a_m)):
            ctx.set_steering(d_sr, a)
            ctx.field_plan(origin, spacing, (n, n, n), F0, C, RHO, P0, flags=nat.OUT_PMAG)
            ctx.field_set_medium(vol["sound_speed"], vol["attenuation"], vol["density"], model=model)
            variant = ctx.field_variant()
            ctx.field_launch()
            p = np.array([ctx.field_fetch(f, want=("pmag",))["pmag"][tuple(idx[f])] for f in range(len(foci))])
            q[name] = p / np.sqrt((a * a).sum(axis=1))
        g = q["matched"] / q["uniform"]
        print(f"{model} ({variant}): |p(focus)| / sqrt(sum apod^2), matched + spreading / Uniform = {g.min():.5f} .. {g.max():.5f}, mean {g.mean():.5f}", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
