"""fp64 oracle of the pulsed model's waveforms and pulse intensity integral: every sample's pressure is the
brute-force sum over the elements active at that sample, with the arrival steps and the activity rule of tests/pulsed_oracle.py
(``ceil(u) <= k < ceil(u + T / dt)``, u = t_e / dt).  Nothing here is shared with the kernel's difference-array scheme.

    p(v, t_k)  = sum_e w_e exp(-a d_e) / d_e cos(2 pi f0 (t_k - t_e)) 1[0 <= t_k - t_e < T],   k = 0 .. n_t - 1
    PII(v)     = 1e-4 dt / (rho c) sum_k p(v, t_k)^2   [J/cm^2]
"""
from __future__ import annotations

import numpy as np

from pulsed_oracle import arrival_steps


def pulsed_waveforms(pts, pos_m, area, delays, apod, freq, c, p0, cycles, dt, n_t, dmin, absorption=0.0, chunk=64, kblock=64):
    """(p [V, n_t], margin [V]) at the points pts [V, 3] [m], fp64.  margin as pulsed_oracle.pulsed_points: the smallest distance of any
    t_e / dt or (t_e + T) / dt of a driven element to an integer."""
    pts = np.atleast_2d(np.asarray(pts, dtype=np.float64))
    pos_m = np.asarray(pos_m, dtype=np.float64)
    w = np.asarray(apod, dtype=np.float64) * np.asarray(area, dtype=np.float64) * p0 * freq / c
    live = w != 0
    tdt = cycles / (freq * dt)
    V, n_t = pts.shape[0], int(n_t)
    p, margin = np.zeros((V, n_t)), np.full(V, np.inf)
    if not live.any():
        return p, margin
    k = np.arange(n_t, dtype=np.float64)
    a = 2.0 * np.pi * ((freq * dt * k) % 1.0)
    ca, sa = np.cos(a), np.sin(a)
    for s in range(0, V, chunk):
        u, d = arrival_steps(pts[s:s + chunk], pos_m[live], np.asarray(delays, dtype=np.float64)[live], dt, c, dmin)
        amp = w[live][None, :] * np.exp(-absorption * d) / d
        for x in (u, u + tdt):
            margin[s:s + chunk] = np.minimum(margin[s:s + chunk], np.abs(x - np.rint(x)).min(1))
        k0, k1 = np.ceil(u), np.ceil(u + tdt)
        b = 2.0 * np.pi * ((freq * dt * u) % 1.0)
        cb, sb = amp * np.cos(b), amp * np.sin(b)
        lo, hi = int(max(0, k0.min())), int(min(n_t, k1.max()))          # (no element is active outside: p stays 0 there)
        for kb in range(lo, hi, kblock):
            kk = k[kb:min(kb + kblock, hi)]
            act = ((kk[None, :, None] >= k0[:, None, :]) & (kk[None, :, None] < k1[:, None, :])).astype(np.float64)      # [V, K, N]
            sc, ss = (act @ cb[:, :, None])[..., 0], (act @ sb[:, :, None])[..., 0]
            p[s:s + chunk, kb:kb + kk.size] = ca[None, kb:kb + kk.size] * sc + sa[None, kb:kb + kk.size] * ss
    return p, margin


def pulsed_pii(pts, pos_m, area, delays, apod, freq, c, rho, p0, cycles, dt, n_t, dmin, absorption=0.0, chunk=64):
    """(PII [V] in J/cm^2, margin [V]): 1e-4 dt / (rho c) sum_k p(t_k)^2 of ``pulsed_waveforms``."""
    pts = np.atleast_2d(np.asarray(pts, dtype=np.float64))
    pii, margin = np.zeros(pts.shape[0]), np.full(pts.shape[0], np.inf)
    for s in range(0, pts.shape[0], 1024):        # (bounds the [V, n_t] block held at once)
        p, m = pulsed_waveforms(pts[s:s + 1024], pos_m, area, delays, apod, freq, c, p0, cycles, dt, n_t, dmin, absorption, chunk)
        pii[s:s + 1024] = 1e-4 * dt / (rho * c) * (p * p).sum(1)
        margin[s:s + 1024] = m
    return pii, margin


def pulsed_pii_grid(xs, ys, zs, pos_m, area, delays, apod, freq, c, rho, p0, cycles, dt, n_t, absorption=0.0):
    """(PII, margin) on the grid xs x ys x zs [m] (C order [nx, ny, nz]); dmin = min(spacing) / 2 as the kernels."""
    sp = [float(v[1] - v[0]) for v in (xs, ys, zs) if len(v) > 1]
    dmin = 0.5 * min(sp) if sp else 0.0
    X, Y, Z = np.meshgrid(xs, ys, zs, indexing="ij")
    pts = np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1)
    out = pulsed_pii(pts, pos_m, area, delays, apod, freq, c, rho, p0, cycles, dt, n_t, dmin, absorption)
    shape = (len(xs), len(ys), len(zs))
    return tuple(o.reshape(shape) for o in out)
