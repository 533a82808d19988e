"""fp64 NumPy restatement of the MediumCompensated apodization (DESIGN.md section 2 "MediumCompensated"), independent of kernel 1a.

For a focus r_f and element e, with g_e, d_e, dz, the plane set k, the crossing samples, the focus sample, l and dmin exactly as in the StraightRay
definition (tests/medium_delay_oracle.py), over the attenuation volume:
    a    = alpha f_MHz^0.9 100 / 8.685889638065035 [Np/m], fp64 from the float32 volume (dB/cm/MHz^0.9)
    A_e  = 0 if dz == 0, else l (a~(r_f) / 2 + sum_k a_k(crossing_k)),   l = hz max(d_e, dmin) / |dz|
    h_e  = exp(-A_e)  [S_e / max(d_e, dmin) with spreading]
    active = {e : b_e > 0} (b = the base method's apodization)
    "equalize": apod_e = b_e (min_active h / h_e)        "matched": apod_e = b_e (h_e / max_active h)        no active element: apod = b."""
from __future__ import annotations

import numpy as np

from medium_delay_oracle import bilinear, element_positions, trilinear

ZTOL = 1e-6             # [plane spacings]
ALPHA_POWER = 0.9
NEPER_DB = 8.685889638065035


def np_per_m(attenuation_db_cm_mhz, freq_hz):
    """a [Np/m] in fp64 from the float32 volume."""
    a = np.asarray(attenuation_db_cm_mhz, dtype=np.float32).astype(np.float64)
    return a * (float(freq_hz) * 1e-6) ** ALPHA_POWER * 100.0 / NEPER_DB


def ray_sums(a, origin, spacing, g, focus):
    """(A_e [Np], d_e [m]) for elements at g [N, 3] (already transformed) and one focus [3] through a [nx, ny, nz] [Np/m]."""
    a = np.asarray(a, dtype=np.float64)
    nx, ny, nz = a.shape
    ox, oy, oz = (float(v) for v in origin)
    hx, hy, hz = (float(v) for v in spacing)
    dmin = 0.5 * min(hx, hy, hz)
    fx, fy, fz = (float(v) for v in focus)
    zs = oz + np.arange(nz) * hz
    af = trilinear(a, (fx - ox) / hx, (fy - oy) / hy, (fz - oz) / hz)
    A, d = np.zeros(len(g)), np.zeros(len(g))
    for e in range(len(g)):
        vx, vy, vz = fx - g[e, 0], fy - g[e, 1], fz - g[e, 2]
        d[e] = np.sqrt(vx * vx + vy * vy + vz * vz)
        if vz == 0:
            continue
        total = 0.5 * af
        for k in range(nz):
            t = (zs[k] - g[e, 2]) / vz
            if not (0 < t < 1) or abs(zs[k] - fz) <= ZTOL * hz:
                continue
            total += bilinear(a[:, :, k], (g[e, 0] + t * vx - ox) / hx, (g[e, 1] + t * vy - oy) / hy)
        A[e] = hz * max(d[e], dmin) / abs(vz) * total
    return A, d


def arrival(pos_m, foci_m, attenuation, origin, spacing, freq_hz, area=None, M=None):
    """(A [F, N], h [F, N], d [F, N]); attenuation None = none; area given = spreading (h = exp(-A) S / max(d, dmin))."""
    g = element_positions(pos_m, M)
    foci = np.atleast_2d(np.asarray(foci_m, dtype=np.float64))
    dmin = 0.5 * min(float(v) for v in spacing)
    A, d = np.zeros((len(foci), len(g))), np.zeros((len(foci), len(g)))
    for f, r in enumerate(foci):
        if attenuation is None:
            d[f] = np.linalg.norm(r - g, axis=1)
        else:
            A[f], d[f] = ray_sums(np_per_m(attenuation, freq_hz), origin, spacing, g, r)
    h = np.exp(-A)
    if area is not None:
        h = h * np.asarray(area, dtype=np.float64)[None, :] / np.maximum(d, dmin)
    return A, h, d


def compensate(b, h, mode):
    """apod [F, N] from the base apodization b and the arrival amplitudes h."""
    if mode not in ("equalize", "matched"):
        raise ValueError(mode)
    b, h = np.atleast_2d(np.asarray(b, dtype=np.float64)), np.atleast_2d(np.asarray(h, dtype=np.float64))
    out = b.copy()
    for f in range(len(b)):
        act = b[f] > 0
        if not act.any():
            continue
        out[f, act] = b[f, act] * (h[f, act].min() / h[f, act] if mode == "equalize" else h[f, act] / h[f, act].max())
    return out


def apodization(pos_m, foci_m, b, attenuation, origin, spacing, freq_hz, mode="equalize", area=None, M=None):
    """MediumCompensated apodization [F, N] over the base apodization b [F, N]."""
    _, h, _ = arrival(pos_m, foci_m, attenuation, origin, spacing, freq_hz, area=area, M=M)
    return compensate(b, h, mode)
