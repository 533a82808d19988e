"""fp64 NumPy restatement of the StraightRay delays (DESIGN.md section 2 "StraightRay"), independent of kernel 1m.

For a focus r_f and element e: g_e = (M [p_e, 1])[:3], d_e = |r_f - g_e|, tof_e = d_e / c_ref, dz = z_f - z_e and
    E_e = 0 if dz == 0, else l (sig~(r_f) / 2 + sum_k sig_k(crossing_k)),   l = hz max(d_e, dmin) / |dz|,  dmin = min(spacing) / 2
    tau_e = tof_e + E_e / c_ref,   delays = max_e tau_e - tau_e
sig = c_ref / c - 1 in fp64 from the float32 sound speed; k runs over the grid planes z_k = z0 + k hz with t = (z_k - z_e) / dz strictly inside
(0, 1) and |z_k - z_f| > 1e-6 hz (a plane that close is the focus' own plane); sig_k is the bilinear, border-extended sample of plane k where
the ray crosses it (oracle/field_oracle.c bilinear2) and sig~ the trilinear, border-extended sample at the focus."""
from __future__ import annotations

import numpy as np

ZTOL = 1e-6     # [plane spacings]


def sigma(sound_speed, c_ref):
    """c_ref / c - 1 in fp64 from the float32 volume."""
    return float(c_ref) / np.asarray(sound_speed, dtype=np.float32).astype(np.float64) - 1.0


def _corners(u, n):
    u = np.clip(u, 0.0, n - 1)
    i0 = np.floor(u).astype(np.int64)
    i0 = np.minimum(i0, max(n - 2, 0))
    i1 = np.where(i0 + 1 < n, i0 + 1, i0)
    return i0, i1, u - i0


def bilinear(plane, u, v):
    """plane [nx, ny] at fractional indices (u, v) (arrays), edge-clamped: bilinear2 of oracle/field_oracle.c."""
    nx, ny = plane.shape
    i0, i1, fu = _corners(np.asarray(u, dtype=np.float64), nx)
    j0, j1, fv = _corners(np.asarray(v, dtype=np.float64), ny)
    return (1 - fu) * ((1 - fv) * plane[i0, j0] + fv * plane[i0, j1]) + fu * ((1 - fv) * plane[i1, j0] + fv * plane[i1, j1])


def trilinear(sig, u, v, w):
    nz = sig.shape[2]
    k0, k1, fw = _corners(np.asarray(w, dtype=np.float64), nz)
    return (1 - fw) * bilinear(sig[:, :, int(k0)], u, v) + fw * bilinear(sig[:, :, int(k1)], u, v)


def element_positions(pos_m, M=None):
    pos = np.asarray(pos_m, dtype=np.float64).reshape(-1, 3)
    if M is None:
        return pos
    M = np.asarray(M, dtype=np.float64)
    return pos @ M[:3, :3].T + M[:3, 3]


def extra_path(sig, origin, spacing, g, focus):
    """E_e [m] for elements at g [N, 3] (already transformed) and one focus [3]."""
    sig = np.asarray(sig, dtype=np.float64)
    nx, ny, nz = sig.shape
    ox, oy, oz = (float(v) for v in origin)
    hx, hy, hz = (float(v) for v in spacing)
    dmin = 0.5 * min(hx, hy, hz)
    fx, fy, fz = (float(v) for v in focus)
    zs = oz + np.arange(nz) * hz
    sf = trilinear(sig, (fx - ox) / hx, (fy - oy) / hy, (fz - oz) / hz)
    vx, vy, vz = fx - g[:, 0], fy - g[:, 1], fz - g[:, 2]
    d = np.sqrt(vx * vx + vy * vy + vz * vz)
    E = np.zeros(len(g))
    for e in np.nonzero(vz != 0)[0]:
        t = (zs - g[e, 2]) / vz[e]
        ks = np.nonzero((t > 0) & (t < 1) & (np.abs(zs - fz) > ZTOL * hz))[0]
        ssum = 0.5 * sf
        for k in ks:
            ssum += bilinear(sig[:, :, k], (g[e, 0] + t[k] * vx[e] - ox) / hx, (g[e, 1] + t[k] * vy[e] - oy) / hy)
        E[e] = hz * max(d[e], dmin) / abs(vz[e]) * ssum
    return E


def delays(pos_m, foci_m, sound_speed, origin, spacing, c_ref, M=None):
    """StraightRay delays [F, N] [s]; sound_speed None = c_ref everywhere (then these are Direct's delays)."""
    g = element_positions(pos_m, M)
    foci = np.atleast_2d(np.asarray(foci_m, dtype=np.float64))
    out = np.empty((len(foci), len(g)))
    for f, r in enumerate(foci):
        tof = np.linalg.norm(r - g, axis=1) / c_ref
        E = np.zeros(len(g)) if sound_speed is None else extra_path(sigma(sound_speed, c_ref), origin, spacing, g, r)
        tau = tof + E / c_ref
        out[f] = tau.max() - tau
    return out
