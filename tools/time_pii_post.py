#!/usr/bin/env python3
"""Time pii_post_k (olx_pii_post's pass over the resident pulse intensity integrals) with HIP events: the scale-only form, V (8 F + 4) bytes --
max_f PII_f is always stored -- and the full form (factors, weights, peaks), V (8 F + 8) bytes; median of the launches after warm-up, as a
fraction of 8 TB/s.  The volumes are uploaded (olx_pii_upload onto an uploaded grid): the pass is HBM-bound whatever the values.

  python tools/time_pii_post.py [--n 256] [--foci 8] [--iters 60] [--warmup 10]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "openlifu-python_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from openlifu_amd import _native as nat      # noqa: E402

HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[256], help="grid n x n x n, or nx ny nz")
    ap.add_argument("--foci", type=int, default=8)
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    n = tuple(a.n * 3) if len(a.n) == 1 else tuple(a.n)
    F = a.foci
    ctx = nat.Context(0)
    rng = np.random.default_rng(5)
    vol = rng.random((F,) + n, dtype=np.float32)
    origin = [-(n[0] - 1) / 2 * 0.5e-3, -(n[1] - 1) / 2 * 0.5e-3, 5e-3]
    ctx.field_upload(origin, [0.5e-3] * 3, n, vol, vol)
    ctx.pii_upload(vol)
    out = {"grid": list(n), "foci": F, "iters": a.iters}
    for form in ("pii_scale", "pii_full"):
        ctx.scan_time(form, a.warmup)
        ms, nbytes = ctx.scan_time(form, a.iters)
        med = float(np.median(ms))
        out[form] = {"median_us": round(med * 1e3, 2), "min_us": round(float(ms.min()) * 1e3, 2), "bytes": nbytes,
                     "TB_per_s": round(nbytes / (med * 1e-3) / 1e12, 3), "fraction_of_8TBps": round(nbytes / (med * 1e-3) / HBM_BYTES_PER_S, 4)}
    assert np.array_equal(ctx.pii_fetch(F), vol)      # (factors of 1.0f: the volumes are as uploaded)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
