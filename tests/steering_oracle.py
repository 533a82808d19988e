"""fp64 NumPy restatement of the steering map (DESIGN.md section 2 "Steering map"), chunked over voxels.

Per voxel v at r_v = origin + index spacing and element e (position g_e, unit normal n_e, area S_e), in the array frame:
    w = r_v - g_e,  d = |w|,  d' = max(d, dmin),  dmin = min(spacing) / 2
    s = |w x n_e| / d (0 at d = 0),  theta = arcsin(min(s, 1))
    a_e = uniform: value | maxangle: 1[theta <= theta_max] | piecewise: clip((zero - theta) / (zero - rolloff), 0, 1)
    P(v) = (P0 / lambda) sum_e a_e S_e D_e(v) exp(-alpha d') / d',   n_active(v) = #{ e : a_e > 0 }
The decision of maxangle (and the a_e > 0 decision of piecewise, theta < zero) is taken as |w x n|^2 <= (<) sin^2(limit) |w|^2, a limit
>= 90 deg passing everything; a voxel is EXCLUDED from bit-exact comparisons of n_active when some element sits on the decision's edge:
| |w x n|^2 - sin^2(limit) |w|^2 | <= 1e-9 |w|^2 with |w| > 0 (at w = 0 exactly the angle is 0 by definition: nothing to round)."""
import numpy as np

from oracle.field_oracle import piston_directivity

EDGE = 1e-9


def steering_map(xs_m, ys_m, zs_m, pos_m, normal, area_m2, freq, c, p0_pa=1.0, apod=("uniform", 1.0, 0.0), radians=False,
                 absorption=0.0, directivity=None, spacing=None, chunk=4096):
    """(P [nx,ny,nz] float64, n_active [nx,ny,nz] int32, excluded [nx,ny,nz] bool).  ``apod`` = (kind, p0, p1) with angles in degrees
    (radians with ``radians``); ``directivity`` = (xaxis [N,3], size_m [N,2]) switches the piston factor on.  The coordinate vectors
    are uniformly spaced: origin + index * spacing; ``spacing`` (3 values [m]) names the steps the clamp dmin = min(spacing) / 2 is
    taken from when an axis has a single voxel (default: the steps of the axes that have more, 0 when none has)."""
    xs, ys, zs = (np.asarray(v, dtype=np.float64) for v in (xs_m, ys_m, zs_m))
    sp = [v[1] - v[0] for v in (xs, ys, zs) if len(v) > 1] if spacing is None else list(spacing)
    dmin = 0.5 * min(sp) if sp else 0.0
    pos = np.asarray(pos_m, dtype=np.float64)
    nrm = np.asarray(normal, dtype=np.float64)
    nrm = nrm / np.sqrt((nrm * nrm).sum(axis=1))[:, None]
    amp = np.asarray(area_m2, dtype=np.float64) * p0_pa * freq / c
    kind, p0, p1 = apod
    to_rad = 1.0 if radians else np.pi / 180.0
    lim = p0 * to_rad
    X, Y, Z = np.meshgrid(xs, ys, zs, indexing="ij")
    pts = np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1)
    V = pts.shape[0]
    P = np.zeros(V); na = np.zeros(V, dtype=np.int32); excl = np.zeros(V, dtype=bool)
    for s0 in range(0, V, chunk):
        w = pts[s0:s0 + chunk, None, :] - pos[None, :, :]
        d2 = (w * w).sum(axis=2)
        d = np.sqrt(d2)
        dc = np.maximum(d, dmin)
        if kind == "uniform":
            a = np.full(d.shape, float(p0))
        else:
            cr = np.cross(w, nrm[None, :, :])
            c2 = (cr * cr).sum(axis=2)
            if lim >= np.pi / 2 and (kind == "maxangle" or lim > np.pi / 2):
                act = np.ones(d.shape, dtype=bool)
            else:
                s2 = np.sin(lim) ** 2
                act = (c2 <= s2 * d2) if kind == "maxangle" else ((c2 < s2 * d2) | (d2 == 0))
                excl[s0:s0 + chunk] = ((np.abs(c2 - s2 * d2) <= EDGE * d2) & (d2 > 0)).any(axis=1)
            if kind == "maxangle":
                a = act.astype(np.float64)
            else:
                sn = np.divide(np.sqrt(c2), d, out=np.zeros_like(d), where=d > 0)
                theta = np.arcsin(np.minimum(sn, 1.0))
                a = np.clip((lim - theta) / ((p0 - p1) * to_rad), 0.0, 1.0) * act
        term = a * amp[None, :] / dc
        if directivity is not None:
            term = term * piston_directivity(w, dc, directivity[0], nrm, directivity[1], freq, c)
        if absorption:
            term = term * np.exp(-absorption * dc)
        P[s0:s0 + chunk] = term.sum(axis=1)
        na[s0:s0 + chunk] = (a > 0).sum(axis=1) if kind != "uniform" else (d.shape[1] if p0 > 0 else 0)
    shape = (len(xs), len(ys), len(zs))
    return P.reshape(shape), na.reshape(shape), excl.reshape(shape)
