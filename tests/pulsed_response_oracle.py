"""fp64 oracle of the pulsed model driven through impulse responses (DESIGN.md section 2 "drive taps", kernel 2p's RESP instantiations):
a brute-force sum over (element, tap) pairs.  Pair (e, m) is element e's burst delayed by m whole steps and scaled by g_e[m]: its arrival
step is u_{e,m} = u_e + m with u_e = t_e / dt of tests/pulsed_oracle.arrival_steps, and it is active at the samples
``ceil(u_e) + m <= k < ceil(u_e + T / dt) + m`` -- the integer shift is applied to the integers of the plain model, tau~ + m dt is never
formed and floored again.  Nothing here is shared with the kernel's FIR form: no envelope, no convolution, every sample's pressure is the
direct sum of the pair terms active at that sample.

    p(v, t_k) = sum_e w_e exp(-a d_e) / d_e sum_m g_e[m] cos(2 pi f0 (t_k - t_e - m dt)) 1[0 <= t_k - t_e - m dt < T],   k = 0 .. n_t - 1
    PII(v)    = 1e-4 dt / (rho c) sum_k p(v, t_k)^2   [J/cm^2]
"""
from __future__ import annotations

import numpy as np

from pulsed_oracle import arrival_steps


def response_waveforms(pts, pos_m, area, delays, apod, cls, taps, freq, c, p0, cycles, dt, n_t, dmin, absorption=0.0, chunk=128):
    """(p [V, n_t], margin [V]) at the points pts [V, 3] [m], fp64.  ``cls`` [N]: class of each element, ``taps``: one array of drive
    taps per class.  margin is pulsed_wave_oracle.pulsed_waveforms' own: the smallest distance of any t_e / dt or (t_e + T) / dt of a
    driven element to an integer (the taps shift both by whole steps: the distance stays)."""
    pts = np.atleast_2d(np.asarray(pts, dtype=np.float64))
    pos_m = np.asarray(pos_m, dtype=np.float64)
    delays = np.asarray(delays, dtype=np.float64)
    cls = np.asarray(cls)
    w = np.asarray(apod, dtype=np.float64) * np.asarray(area, dtype=np.float64) * p0 * freq / c
    live = w != 0
    tdt = cycles / (freq * dt)
    V, n_t = pts.shape[0], int(n_t)
    p, margin = np.zeros((V, n_t)), np.full(V, np.inf)
    if not live.any():
        return p, margin
    k = np.arange(n_t)
    for s in range(0, V, chunk):
        u, d = arrival_steps(pts[s:s + chunk], pos_m[live], delays[live], dt, c, dmin)
        for x in (u, u + tdt):
            margin[s:s + chunk] = np.minimum(margin[s:s + chunk], np.abs(x - np.rint(x)).min(1))
        amp = w[live][None, :] * np.exp(-absorption * d) / d
        k0, k1 = np.ceil(u).astype(np.int64), np.ceil(u + tdt).astype(np.int64)
        blk = p[s:s + chunk]
        for r, g in enumerate(taps):
            sel = cls[live] == r
            if not sel.any():
                continue
            ur, ar, k0r, k1r = u[:, sel], amp[:, sel], k0[:, sel], k1[:, sel]
            for m, gm in enumerate(np.asarray(g, dtype=np.float64)):
                if gm == 0.0 or k0r.min() + m >= n_t:
                    continue
                lo, hi = max(0, int(k0r.min()) + m), min(n_t, int(k1r.max()) + m)      # (no pair of this tap is active outside)
                kk = k[lo:hi]
                act = (kk[None, :, None] >= k0r[:, None, :] + m) & (kk[None, :, None] < k1r[:, None, :] + m)      # [V, K, Nr]
                # cos(2 pi f0 dt (k - u_{e,m})), both arguments reduced modulo one period
                a = 2.0 * np.pi * ((freq * dt * kk) % 1.0)
                b = 2.0 * np.pi * ((freq * dt * (ur + m)) % 1.0)
                cs = act.astype(np.float64) @ np.stack([gm * ar * np.cos(b), gm * ar * np.sin(b)], axis=-1)      # [V, K, 2]
                blk[:, lo:hi] += np.cos(a)[None, :] * cs[..., 0] + np.sin(a)[None, :] * cs[..., 1]
    return p, margin


def response_volumes(pts, pos_m, area, delays, apod, cls, taps, freq, c, rho, p0, cycles, dt, n_t, dmin, absorption=0.0):
    """dict(p [V, n_t], pmax, pmin, pii [J/cm^2], margin), each [V]: p_max = max(0, max_k p), p_min = max(0, -min_k p), PII as above."""
    p, margin = response_waveforms(pts, pos_m, area, delays, apod, cls, taps, freq, c, p0, cycles, dt, n_t, dmin, absorption)
    return dict(p=p, pmax=np.maximum(p.max(1), 0.0), pmin=np.maximum(-p.min(1), 0.0), pii=1e-4 * dt / (rho * c) * (p * p).sum(1), margin=margin)
