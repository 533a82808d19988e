"""fp64 oracle of the pulsed (tone-burst) field model through a heterogeneous medium along straight rays (DESIGN.md section 2 "Pulsed model
through a medium", kernel 2ph): the brute-force sum over samples k and elements e of tests/pulsed_oracle.py, with the ray sums A_e [Np] and
E_e [m] of tests/steering_medium_oracle.py (``medium_sums``: kernel 4h's definition at a grid voxel) on every (voxel, element) ray.  Nothing here
is shared with the kernel's difference-array scheme, its register cache or its medium layout.

    t_e       = floor(tau_e / dt) dt + (d'_e + E_e) / c_ref,        d'_e = max(|r_v - g_e|, dmin),  w_e = a_e P0 S_e f0 / c_ref
    p(v, t_k) = sum_e w_e exp(-A_e) / d'_e cos(2 pi f0 (t_k - t_e)) 1[0 <= t_k - t_e < T],   T = cycles / f0,  t_k = k dt
    p_max = max(0, max_k p),  p_min = max(0, -min_k p),  intensity = 1e-4 p_min^2 / (2 rho(v) c(v)),  PII = 1e-4 dt / (rho(v) c(v)) sum_k p^2

The voxels are grid voxels (integer indices; r_v = origin + index spacing), as the ray sums are defined there.
"""
from __future__ import annotations

import numpy as np

import steering_medium_oracle as smo


def voxel_indices(n, voxels=None):
    """[V, 3] integer indices: ``voxels`` as given, None = the whole grid in C order."""
    if voxels is not None:
        return np.atleast_2d(np.asarray(voxels, dtype=np.int64))
    nx, ny, nz = (int(v) for v in n)
    return np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), axis=-1).reshape(-1, 3)


def ray_sums(origin, spacing, n, pos_m, freq, c_ref, sound_speed=None, attenuation=None, voxels=None):
    """(A [V, N] Np, E [V, N] m) of tests/steering_medium_oracle.py for the voxels (None = the whole grid)."""
    return smo.medium_sums(origin, spacing, n, pos_m, freq, c_ref, sound_speed, attenuation, None if voxels is None else voxel_indices(n, voxels))


def arrival_steps(pts, pos_m, delays, dt, c, dmin, E):
    """u = t_e / dt [V, N] = (tau~ + (d' + E) / c_ref) / dt in that order of operations (E == 0.0 gives pulsed_oracle.arrival_steps' u bit
    for bit) and the clamped distances d' [V, N]."""
    d = np.sqrt(((pts[:, None, :] - pos_m[None, :, :]) ** 2).sum(-1))
    d = np.maximum(d, dmin)
    tau = np.floor(np.asarray(delays, dtype=np.float64) / dt) * dt
    return (tau[None, :] + (d + E) / c) / dt, d


def _points(origin, spacing, idx):
    return np.asarray(origin, dtype=np.float64)[None, :] + idx * np.asarray(spacing, dtype=np.float64)[None, :]


def pulsed_medium(origin, spacing, n, pos_m, area, delays, apod, freq, c, p0, cycles, dt, n_t, A, E, voxels=None, chunk=256, kblock=64):
    """(p_max, p_min, margin) [V] at the voxels (None = the whole grid, C order), fp64; A, E [V, N] = ``ray_sums`` of the same voxels.
    margin = the smallest distance of any t_e / dt or (t_e + T) / dt of a driven element to an integer."""
    idx = voxel_indices(n, voxels)
    pts = _points(origin, spacing, idx)
    pos_m = np.asarray(pos_m, dtype=np.float64)
    dmin = 0.5 * min(float(v) for v in spacing)
    w = np.asarray(apod, dtype=np.float64) * np.asarray(area, dtype=np.float64) * p0 * freq / c
    tdt = cycles / (freq * dt)
    V = pts.shape[0]
    pmax, pmin, margin = np.zeros(V), np.zeros(V), np.full(V, np.inf)
    live = w != 0
    for s in range(0, V, chunk):
        u, d = arrival_steps(pts[s:s + chunk], pos_m, delays, dt, c, dmin, E[s:s + chunk])
        amp = w[None, :] * np.exp(-A[s:s + chunk]) / d
        amp = np.where(w[None, :] != 0, amp, 0.0)
        k0, k1 = np.ceil(u), np.ceil(u + tdt)
        for x in (u, u + tdt):
            margin[s:s + chunk] = np.minimum(margin[s:s + chunk], np.where(w[None, :] != 0, np.abs(x - np.rint(x)), np.inf).min(1))
        if not live.any():
            continue
        lo = int(max(0, k0[:, live].min()))
        hi = int(min(n_t, k1[:, live].max()))
        mx, mn = np.zeros(u.shape[0]), np.zeros(u.shape[0])
        for kb in range(lo, hi, kblock):
            k = np.arange(kb, min(kb + kblock, hi), dtype=np.float64)
            act = ((k[None, :, None] >= k0[:, None, :]) & (k[None, :, None] < k1[:, None, :])).astype(np.float64)    # [V, K, N]
            a = 2.0 * np.pi * ((freq * dt * k) % 1.0)
            b = 2.0 * np.pi * ((freq * dt * u) % 1.0)
            sc, ss = (act @ (amp * np.cos(b))[:, :, None])[..., 0], (act @ (amp * np.sin(b))[:, :, None])[..., 0]
            p = np.cos(a)[None, :] * sc + np.sin(a)[None, :] * ss
            mx = np.maximum(mx, p.max(1))
            mn = np.minimum(mn, p.min(1))
        pmax[s:s + chunk], pmin[s:s + chunk] = mx, -mn
    return pmax, pmin, margin


def pulsed_medium_waveforms(origin, spacing, n, pos_m, area, delays, apod, freq, c, p0, cycles, dt, n_t, A, E, voxels=None, chunk=64, kblock=64):
    """(p [V, n_t], margin [V]): every sample's pressure as the brute-force sum over the elements active at it (tests/pulsed_wave_oracle.py's
    form) -- the waveforms of the traces, and sum_k p^2 of the PII."""
    idx = voxel_indices(n, voxels)
    pts = _points(origin, spacing, idx)
    pos_m = np.asarray(pos_m, dtype=np.float64)
    dmin = 0.5 * min(float(v) for v in spacing)
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
        u, d = arrival_steps(pts[s:s + chunk], pos_m[live], np.asarray(delays, dtype=np.float64)[live], dt, c, dmin, E[s:s + chunk][:, live])
        amp = w[live][None, :] * np.exp(-A[s:s + chunk][:, live]) / d
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


def impedance(n, rho, c, sound_speed=None, density=None, voxels=None):
    """rho(v) c(v) [V] from the float32 volumes (None = the constant)."""
    idx = voxel_indices(n, voxels)
    cs = np.full(len(idx), float(c)) if sound_speed is None else np.asarray(sound_speed, dtype=np.float32).astype(np.float64)[tuple(idx.T)]
    rh = np.full(len(idx), float(rho)) if density is None else np.asarray(density, dtype=np.float32).astype(np.float64)[tuple(idx.T)]
    return rh * cs


def pulsed_medium_pii(p, dt, z):
    """PII [V] in J/cm^2 = 1e-4 dt / (rho c) sum_k p(t_k)^2 of the waveforms p [V, n_t] and the impedance z [V]."""
    return 1e-4 * dt / z * (p * p).sum(1)
