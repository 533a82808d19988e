"""fp64 oracle of the pulsed (tone-burst) field model (kernel 2p): a brute-force NumPy sum over samples k and
elements e, chunked over voxels.  Nothing here is shared with the kernel's difference-array scheme: every sample's pressure is the
direct sum of the element terms active at that sample.

    p(v, t_k) = sum_e w_e exp(-a d_e) / d_e cos(2 pi f0 (t_k - t_e)) 1[0 <= t_k - t_e < T]
    t_e = floor(tau_e / dt) dt + d_e / c,  T = cycles / f0,  t_k = k dt,  d_e = max(|r_v - r_e|, dmin),  w_e = a_e P0 S_e f0 / c
"""
from __future__ import annotations

import numpy as np


def arrival_steps(pts, pos_m, delays, dt, c, dmin):
    """t_e / dt [V, N] of voxels pts [V, 3] (fp64, the definition's order of operations) and the clamped distances d [V, N]."""
    d = np.sqrt(((pts[:, None, :] - pos_m[None, :, :]) ** 2).sum(-1))
    d = np.maximum(d, dmin)
    tau = np.floor(np.asarray(delays, dtype=np.float64) / dt) * dt
    return (tau[None, :] + d / c) / dt, d


def pulsed_points(pts, pos_m, area, delays, apod, freq, c, p0, cycles, dt, n_t, dmin, absorption=0.0, chunk=256, kblock=64):
    """(p_max, p_min, margin) at the points pts [V, 3] [m], fp64.  margin = the smallest distance of any t_e / dt or (t_e + T) / dt
    to an integer (where an fp32 / fp64 difference could move an element term across a sample)."""
    pts = np.atleast_2d(np.asarray(pts, dtype=np.float64))
    w = np.asarray(apod, dtype=np.float64) * np.asarray(area, dtype=np.float64) * p0 * freq / c
    tdt = cycles / (freq * dt)
    V = pts.shape[0]
    pmax, pmin, margin = np.zeros(V), np.zeros(V), np.full(V, np.inf)
    for s in range(0, V, chunk):
        u, d = arrival_steps(pts[s:s + chunk], pos_m, delays, dt, c, dmin)
        amp = w[None, :] * np.exp(-absorption * d) / d
        amp = np.where(w[None, :] != 0, amp, 0.0)
        k0, k1 = np.ceil(u), np.ceil(u + tdt)
        for x in (u, u + tdt):
            margin[s:s + chunk] = np.minimum(margin[s:s + chunk], np.where(w[None, :] != 0, np.abs(x - np.rint(x)), np.inf).min(1))
        live = w != 0
        if not live.any():
            continue
        lo = int(max(0, k0[:, live].min()))
        hi = int(min(n_t, k1[:, live].max()))
        mx, mn = np.zeros(u.shape[0]), np.zeros(u.shape[0])
        for kb in range(lo, hi, kblock):
            k = np.arange(kb, min(kb + kblock, hi), dtype=np.float64)
            act = ((k[None, :, None] >= k0[:, None, :]) & (k[None, :, None] < k1[:, None, :])).astype(np.float64)    # [V, K, N]
            # cos(2 pi f0 (t_k - t_e)) = cos(a_k) cos(b_e) + sin(a_k) sin(b_e), a_k = 2 pi f0 dt k, b_e = 2 pi f0 dt u_e (reduced mod 1 period)
            a = 2.0 * np.pi * ((freq * dt * k) % 1.0)
            b = 2.0 * np.pi * ((freq * dt * u) % 1.0)
            sc = (act @ (amp * np.cos(b))[:, :, None])[..., 0], (act @ (amp * np.sin(b))[:, :, None])[..., 0]
            p = np.cos(a)[None, :] * sc[0] + np.sin(a)[None, :] * sc[1]
            mx = np.maximum(mx, p.max(1))
            mn = np.minimum(mn, p.min(1))
        pmax[s:s + chunk], pmin[s:s + chunk] = mx, -mn
    return pmax, pmin, margin


def pulsed_grid(xs, ys, zs, pos_m, area, delays, apod, freq, c, p0, cycles, dt, n_t, absorption=0.0, chunk=256):
    """(p_max, p_min, margin) on the grid xs x ys x zs [m] (C order [nx, ny, nz]); dmin = min(spacing) / 2 as the kernels."""
    sp = [float(v[1] - v[0]) for v in (xs, ys, zs) if len(v) > 1]
    dmin = 0.5 * min(sp) if sp else 0.0
    X, Y, Z = np.meshgrid(xs, ys, zs, indexing="ij")
    pts = np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1)
    out = pulsed_points(pts, pos_m, area, delays, apod, freq, c, p0, cycles, dt, n_t, dmin, absorption, chunk)
    shape = (len(xs), len(ys), len(zs))
    return tuple(o.reshape(shape) for o in out)
