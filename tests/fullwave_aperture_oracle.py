"""fp64 oracle of the full-wave model's rectangular element apertures (DESIGN.md section 2 "full-wave model: apertures"), written from
the definition in SCATTER form: every quadrature point is spread on the 8 corners around it and merged per (element, voxel) in a dict --
deliberately the other formulation from the device's gather (fullwave_aperture_k: one lane per voxel walking the points).  Shares
nothing with the product (openlifu_amd/sim/fullwave.py, csrc/k_fullwave.hip) except inputs; its expanded entries feed
fullwave_oracle.simulate as they are.

Element e: centre c [m], in-plane unit axes u = R[:, 0] (width) and v = R[:, 1] (length), R = Raz(y) Rel(x') Rroll(z''), size (w, l) [m].
Points x_ab = c + ((a + 1/2) / n_w - 1/2) w u + ((b + 1/2) / n_l - 1/2) l v with n_w = max(1, ceil(r w / h_min - 1e-9)), n_l likewise;
q = (x - origin) / h, a coordinate within 1e-9 of a whole number counting as it; W_e(m) = 1 / (n_w n_l) sum_a sum_b prod_axis
max(0, 1 - |q_axis - m_axis|), a outer, b inner."""
import numpy as np

MAX_POINTS = 65536


def rotation(az, el, roll):
    """R = Raz(y) . Rel(x') . Rroll(z''), as a product of the three plane rotations"""
    ca, sa, ce, se, cr, sr = np.cos(az), np.sin(az), np.cos(el), np.sin(el), np.cos(roll), np.sin(roll)
    Raz = np.array([[ca, 0, sa], [0, 1, 0], [-sa, 0, ca]])
    Rel = np.array([[1, 0, 0], [0, ce, -se], [0, se, ce]])
    Rroll = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    return Raz @ Rel @ Rroll


def counts(size, h, rate):
    """(n_w, n_l) of an element of ``size`` = (w, l) [m] on a grid of spacing ``h`` at upsampling rate ``rate``"""
    hmin = float(np.min(np.broadcast_to(np.asarray(h, dtype=np.float64), (3,))))
    return tuple(max(1, int(np.ceil(int(rate) * float(s) / hmin - 1e-9))) for s in size)


def points_q(centre, u, v, size, n_w, n_l, origin, h):
    """q_ab [n_w n_l, 3] in voxel units (a outer, b inner), snapped; each operation rounded on its own, in the order of the definition"""
    h = np.broadcast_to(np.asarray(h, dtype=np.float64), (3,))
    out = np.empty((n_w * n_l, 3))
    w, l = float(size[0]), float(size[1])
    for a in range(n_w):
        sa = (a + 0.5) / n_w - 0.5
        for b in range(n_l):
            sb = (b + 0.5) / n_l - 0.5
            for k in range(3):
                ta = (sa * w) * float(u[k])
                tb = (sb * l) * float(v[k])
                q = (((float(centre[k]) + ta) + tb) - float(origin[k])) / float(h[k])
                near = np.rint(q)
                out[a * n_l + b, k] = near if abs(q - near) <= 1e-9 else q
    return out


def element_weights(centre, u, v, size, n_w, n_l, origin, h, n, name="element"):
    """{(i, j, k): W} of one element, the non-zero weights only, in the order the scatter first meets the voxels"""
    if n_w < 1 or n_l < 1:
        raise ValueError(f"{name}: n_w and n_l must be >= 1")
    if n_w * n_l > MAX_POINTS:
        raise ValueError(f"{name}: {n_w * n_l} points are too many")
    acc = {}
    for q in points_q(centre, u, v, size, n_w, n_l, origin, h):
        lo = np.floor(q).astype(int)
        f = q - lo
        for corner in np.ndindex(2, 2, 2):
            wx, wy, wz = (f[a] if corner[a] else 1.0 - f[a] for a in range(3))
            wt = (wx * wy) * wz
            if wt == 0:
                continue
            m = tuple(int(t) for t in lo + np.array(corner))
            if any(m[a] < 0 or m[a] >= n[a] for a in range(3)):
                raise ValueError(f"{name} does not lie inside the grid (its voxel {m} is outside {tuple(n)})")
            acc[m] = acc.get(m, 0.0) + wt
    return {m: s / (n_w * n_l) for m, s in acc.items() if s != 0}


def aperture_table(centres, axes_u, axes_v, sizes, n_w, n_l, origin, h, n):
    """Per-element CSR -> (row [E + 1], ijk [S, 3], W [S]), the voxels of a row in ascending C order"""
    row, ijk, wt = [0], [], []
    for e in range(len(centres)):
        d = element_weights(centres[e], axes_u[e], axes_v[e], sizes[e], int(n_w[e]), int(n_l[e]), origin, h, n, name=f"element {e}")
        for m in sorted(d):
            ijk.append(m); wt.append(d[m])
        row.append(len(ijk))
    return np.asarray(row, dtype=np.int64), np.asarray(ijk, dtype=np.int64).reshape(-1, 3), np.asarray(wt, dtype=np.float64)


def dense(row, ijk, wt, n):
    """[E, nx, ny, nz] volumes of the weights (a voxel without an entry is 0)"""
    out = np.zeros((len(row) - 1,) + tuple(n))
    for e in range(len(row) - 1):
        for q in range(row[e], row[e + 1]):
            out[(e,) + tuple(ijk[q])] = wt[q]
    return out


def expand(row, ijk, wt, A, tau, c_vol_or_scalar, freq, dt, h, n):
    """Per-entry (ijk, amp, tau) for fullwave_oracle.simulate: entry (e, m) is a monopole of amplitude amp_{e,m} A_e = W_e(m) dt c(m)^2 4 pi A_e /
    (2 pi f h_x h_y h_z) and delay tau_e; element by element, so the entries of one voxel stand in ascending element order"""
    h = np.broadcast_to(np.asarray(h, dtype=np.float64), (3,))
    cvol = np.broadcast_to(np.asarray(c_vol_or_scalar, dtype=np.float64), tuple(n))
    el = np.repeat(np.arange(len(row) - 1), np.diff(row))
    A, tau = np.asarray(A, dtype=np.float64), np.asarray(tau, dtype=np.float64)
    amp = [w * dt * cvol[tuple(m)] ** 2 * 4 * np.pi * A[e] / (2 * np.pi * freq * np.prod(h)) for w, m, e in zip(wt, ijk, el)]
    return ijk, np.array(amp, dtype=np.float64).reshape(-1), tau[el]
