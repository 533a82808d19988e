"""fp64 NumPy restatement of the steering map through a heterogeneous medium (DESIGN.md section 2 "Steering map through a medium"), vectorised
over voxels; independent of kernel 4h.  Built on tests/steering_oracle.py (n_active and the excluded mask are its own) and on the ``bilinear``
of tests/medium_delay_oracle.py.

Candidate target: grid voxel v = (i, j, kv), r_v = origin + index spacing.  Per element e, with w = r_v - g_e, d = |w|, d' = max(d, dmin),
dmin = min(spacing) / 2, the base apodization b_e, S_e and the optional piston factor D_e exactly as in tests/steering_oracle.py:
    z_k    = oz + k hz
    K_e(v) = kfirst_e <= k < kv (voxel above the element) | kv < k <= klast_e (below); kfirst / klast = first / last plane strictly above / below z_e
    A_e    = 0 if z_v == z_e, else l (a(v) / 2 + sum_{k in K} a_k(crossing_k)),   l = hz d' / |z_v - z_e|,   E_e = the same over sig = c_ref / c - 1
    h_e    = exp(-A_e) [S_e / d' with spreading]
    c_e    = b_e (comp None) | b_e min_active(h) / h_e ("equalize") | b_e h_e / max_active(h) ("matched"); active = {b_e > 0}; with a comp mode an
             element that is not active has c_e = 0 (so: no active element, P = 0)
    P      = (P0 / lambda) sum_e c_e S_e D_e exp(-A_e) / d'                                    delays "straight_ray"
           = (P0 / lambda) | sum_e c_e S_e D_e exp(-A_e) / d' exp(j 2 pi E_e / lambda) |       delays "direct";   lambda = c_ref / f
a = kernel 1a's conversion of the float32 attenuation volume (tests/medium_apod_oracle.np_per_m), sig = kernel 1m's (medium_delay_oracle.sigma);
crossing_k = where the ray g_e -> r_v meets plane k, sampled bilinear and border-extended."""
from __future__ import annotations

import numpy as np

from oracle.field_oracle import piston_directivity
from medium_apod_oracle import np_per_m
from medium_delay_oracle import bilinear, sigma
import steering_oracle as so


def grid_axes(origin, spacing, n):
    return tuple(float(origin[a]) + np.arange(int(n[a])) * float(spacing[a]) for a in range(3))


def plane_bounds(zs, ze):
    """(kfirst, klast): first plane strictly above ze (nz when none), last plane strictly below (-1 when none)."""
    above, below = np.nonzero(zs > ze)[0], np.nonzero(zs < ze)[0]
    return (int(above[0]) if len(above) else len(zs)), (int(below[-1]) if len(below) else -1)


def ray_sums(vol, origin, spacing, g, voxels=None):
    """S [V, N]: the straight-ray sum of ``vol`` [nx, ny, nz] (fp64) from every element g [N, 3] to the voxels ([V, 3] integer indices; None = the
    whole grid in C order), in vol's unit times metres."""
    vol = np.asarray(vol, dtype=np.float64)
    nx, ny, nz = vol.shape
    ox, oy, oz = (float(v) for v in origin)
    hx, hy, hz = (float(v) for v in spacing)
    dmin = 0.5 * min(hx, hy, hz)
    if voxels is None:
        voxels = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), axis=-1).reshape(-1, 3)
    iv, jv, kv = (np.asarray(voxels)[:, a].astype(np.int64) for a in range(3))
    xv, yv, zv = ox + iv * hx, oy + jv * hy, oz + kv * hz
    zs = oz + np.arange(nz) * hz
    planes = [k for k in range(nz) if np.any(vol[:, :, k] != 0)]
    own = 0.5 * vol[iv, jv, kv]
    out = np.zeros((len(iv), len(g)))
    for e in range(len(g)):
        wx, wy, wz = xv - g[e, 0], yv - g[e, 1], zv - g[e, 2]
        d = np.sqrt(wx * wx + wy * wy + wz * wz)
        kfirst, klast = plane_bounds(zs, g[e, 2])
        total = own.copy()
        for k in planes:
            sel = ((kv > k) if k >= kfirst else np.zeros(len(kv), dtype=bool)) | ((kv < k) if k <= klast else np.zeros(len(kv), dtype=bool))
            if not sel.any():
                continue
            t = (zs[k] - g[e, 2]) / wz[sel]
            total[sel] += bilinear(vol[:, :, k], (g[e, 0] + t * wx[sel] - ox) / hx, (g[e, 1] + t * wy[sel] - oy) / hy)
        nz_ = wz != 0
        out[nz_, e] = hz * np.maximum(d[nz_], dmin) / np.abs(wz[nz_]) * total[nz_]
    return out


def base_apodization(w, nrm, apod, radians=False):
    """b [V, N] of tests/steering_oracle.py (same expressions) for w [V, N, 3]."""
    kind, p0, p1 = apod
    d2 = (w * w).sum(axis=2)
    if kind == "uniform":
        return np.full(d2.shape, float(p0))
    to_rad = 1.0 if radians else np.pi / 180.0
    lim = p0 * to_rad
    cr = np.cross(w, nrm[None, :, :])
    c2 = (cr * cr).sum(axis=2)
    if lim >= np.pi / 2 and (kind == "maxangle" or lim > np.pi / 2):
        act = np.ones(d2.shape, dtype=bool)
    else:
        s2 = np.sin(lim) ** 2
        act = (c2 <= s2 * d2) if kind == "maxangle" else ((c2 < s2 * d2) | (d2 == 0))
    if kind == "maxangle":
        return act.astype(np.float64)
    d = np.sqrt(d2)
    sn = np.divide(np.sqrt(c2), d, out=np.zeros_like(d), where=d > 0)
    return np.clip((lim - np.arcsin(np.minimum(sn, 1.0))) / ((p0 - p1) * to_rad), 0.0, 1.0) * act


def compensated(b, h, comp):
    """c [V, N] from the base apodization and the arrival amplitudes."""
    if comp is None:
        return b
    if comp not in ("equalize", "matched"):
        raise ValueError(comp)
    act = b > 0
    out = np.zeros_like(b)
    rows = act.any(axis=1)
    if comp == "equalize":
        hmin = np.where(rows, np.where(act, h, np.inf).min(axis=1), 0.0)
        np.divide(b * hmin[:, None], h, out=out, where=act & rows[:, None])
    else:
        hmax = np.where(rows, np.where(act, h, -np.inf).max(axis=1), 1.0)
        np.divide(b * h, hmax[:, None], out=out, where=act & rows[:, None])
    return out


def medium_sums(origin, spacing, n, pos_m, freq, c_ref, sound_speed=None, attenuation=None, voxels=None):
    """(A [V, N] Np, E [V, N] m): the ray sums that depend on the geometry and the medium only -- compute once, share among the modes."""
    g = np.asarray(pos_m, dtype=np.float64)
    shape = (len(g),)
    V = int(np.prod([int(v) for v in n])) if voxels is None else len(voxels)
    A = np.zeros((V,) + shape) if attenuation is None else ray_sums(np_per_m(attenuation, freq), origin, spacing, g, voxels)
    E = np.zeros((V,) + shape) if sound_speed is None else ray_sums(sigma(sound_speed, c_ref), origin, spacing, g, voxels)
    return A, E


def steering_map_medium(origin, spacing, n, pos_m, normal, area_m2, freq, c_ref, p0_pa=1.0, apod=("uniform", 1.0, 0.0), radians=False,
                        sound_speed=None, attenuation=None, comp=None, spreading=False, delays="straight_ray", directivity=None, sums=None):
    """(P [nx,ny,nz] float64, n_active int32, excluded bool).  ``sums`` = medium_sums(...) of the same geometry and medium, when already known."""
    if delays not in ("straight_ray", "direct"):
        raise ValueError(delays)
    xs, ys, zs = grid_axes(origin, spacing, n)
    pos = np.asarray(pos_m, dtype=np.float64)
    nrm = np.asarray(normal, dtype=np.float64)
    nrm = nrm / np.sqrt((nrm * nrm).sum(axis=1))[:, None]
    area = np.asarray(area_m2, dtype=np.float64)
    _, na, excl = so.steering_map(xs, ys, zs, pos, nrm, area, freq, c_ref, p0_pa, apod=apod, radians=radians, spacing=spacing)
    A, E = medium_sums(origin, spacing, n, pos, freq, c_ref, sound_speed, attenuation) if sums is None else sums
    X, Y, Z = np.meshgrid(xs, ys, zs, indexing="ij")
    w = np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1)[:, None, :] - pos[None, :, :]
    d = np.sqrt((w * w).sum(axis=2))
    dc = np.maximum(d, 0.5 * min(float(v) for v in spacing))
    b = base_apodization(w, nrm, apod, radians)
    ea = np.exp(-A)
    h = ea * area[None, :] / dc if spreading else ea
    term = compensated(b, h, comp) * area[None, :] * ea / dc
    if directivity is not None:
        term = term * piston_directivity(w, dc, directivity[0], nrm, directivity[1], freq, c_ref)
    lam = c_ref / freq
    if delays == "direct":
        P = np.abs((term * np.exp(2j * np.pi * E / lam)).sum(axis=1))
    else:
        P = term.sum(axis=1)
    return (p0_pa / lam * P).reshape(na.shape), na, excl
