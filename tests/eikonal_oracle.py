"""fp64 NumPy restatement of the Eikonal delay method (DESIGN.md section 2 "Eikonal"), independent of kernel 6: a vectorised Jacobi
iteration of the first-order upwind (Godunov) update, written from the definition's text.

Grid: origin o, spacing h_a, counts n_a, voxel centres; slowness s = 1 / c.  Source x_t at index coordinates q = (x_t - o) / h.  The
voxels with sqrt(sum_a (i_a - q_a)^2) <= init_radius start at |x_v - x_t| s(v) and are frozen, every other voxel at +inf.  One sweep reads
T_in and writes T_out: per axis m_a = min of the two neighbours (+inf outside the grid); the three (m_a, h_a) sorted by m ascending, ties in
axis order -> (a1, h1), (a2, h2), (a3, h3), w_i = 1 / h_i^2, u_i = a_i - a1; t = a1 + s h1; if a2 < t the two-axis root, if then a3 < t the
three-axis root, each a1 + (B + sqrt(max(B^2 - A C, 0))) / A; T_out = min(T_in, t).  Sweeps repeat until one changes no voxel; that one counts."""
from __future__ import annotations

import numpy as np


def index_coords(x_t, origin, spacing):
    return (np.asarray(x_t, dtype=np.float64) - np.asarray(origin, dtype=np.float64)) / np.asarray(spacing, dtype=np.float64)


def init_set(n, spacing, q, slowness, init_radius):
    """(T0 with +inf outside the init set, frozen mask)"""
    idx = np.meshgrid(*[np.arange(v, dtype=np.float64) for v in n], indexing="ij")
    d = [idx[a] - q[a] for a in range(3)]
    frozen = np.sqrt(d[0] ** 2 + d[1] ** 2 + d[2] ** 2) <= init_radius
    dist = np.sqrt((d[0] * spacing[0]) ** 2 + (d[1] * spacing[1]) ** 2 + (d[2] * spacing[2]) ** 2)
    return np.where(frozen, dist * slowness, np.inf), frozen


def _axis_min(T, a):
    lo = np.full_like(T, np.inf)
    hi = np.full_like(T, np.inf)
    src = [slice(None)] * 3
    dst = [slice(None)] * 3
    dst[a], src[a] = slice(1, None), slice(None, -1)
    lo[tuple(dst)] = T[tuple(src)]
    dst[a], src[a] = slice(None, -1), slice(1, None)
    hi[tuple(dst)] = T[tuple(src)]
    return np.minimum(lo, hi)


def _root(A, B, C):
    return (B + np.sqrt(np.maximum(B * B - A * C, 0.0))) / A


def sweep(T, frozen, slowness, spacing):
    """One Jacobi sweep -> T_out"""
    a = [_axis_min(T, ax) for ax in range(3)]
    hs = [np.full(T.shape, float(spacing[ax])) for ax in range(3)]
    for p, r in ((0, 1), (1, 2), (0, 1)):       # exchanges of neighbours on a strict "less": ascending, ties stay in axis order
        swap = a[r] < a[p]
        a[p], a[r] = np.where(swap, a[r], a[p]), np.where(swap, a[p], a[r])
        hs[p], hs[r] = np.where(swap, hs[r], hs[p]), np.where(swap, hs[p], hs[r])
    w = [1.0 / v ** 2 for v in hs]
    s = slowness
    with np.errstate(invalid="ignore", over="ignore"):
        u2, u3 = a[1] - a[0], a[2] - a[0]
        t = a[0] + s * hs[0]
        two = a[1] < t
        t2 = a[0] + _root(w[0] + w[1], w[1] * u2, w[1] * u2 ** 2 - s ** 2)
        t = np.where(two, t2, t)
        three = two & (a[2] < t)
        t3 = a[0] + _root(w[0] + w[1] + w[2], w[1] * u2 + w[2] * u3, w[1] * u2 ** 2 + w[2] * u3 ** 2 - s ** 2)
        t = np.where(three, t3, t)
        out = np.where(t < T, t, T)      # min(T_in, t); a NaN of an all-infinite neighbourhood keeps T_in
    return np.where(frozen, T, out)


def solve(n, origin, spacing, sound_speed, x_t, init_radius=3.0, max_sweeps=None):
    """(T [nx, ny, nz] fp64, sweeps).  sound_speed: a scalar or a volume (taken as given, in fp64)."""
    n = tuple(int(v) for v in n)
    spacing = np.broadcast_to(np.asarray(spacing, dtype=np.float64), (3,))
    q = index_coords(x_t, origin, spacing)
    if not (np.all(q >= 0) and np.all(q <= np.asarray(n) - 1)):
        raise ValueError(f"target {tuple(x_t)} outside the grid")
    if not init_radius >= 1:
        raise ValueError("init_radius must be >= 1")
    s = 1.0 / np.broadcast_to(np.asarray(sound_speed, dtype=np.float64), n)
    T, frozen = init_set(n, spacing, q, s, init_radius)
    max_sweeps = 4 * sum(n) if max_sweeps is None else int(max_sweeps)
    for k in range(1, max_sweeps + 1):
        Tn = sweep(T, frozen, s, spacing)
        if np.array_equal(Tn, T):
            return T, k
        T = Tn
    raise RuntimeError(f"no convergence within {max_sweeps} sweeps")


def trilinear_table(points_m, origin, spacing, n, snap=1e-9):
    """CSR table (row [P + 1], ijk [S, 3], weight [S]) of the trilinear rule: the 8 voxels around a point, weights of 0 dropped, a position
    within ``snap`` voxels of a voxel centre counts as on it; a weighted voxel outside the grid raises ValueError naming the point."""
    pts = np.atleast_2d(np.asarray(points_m, dtype=np.float64))
    row, ijk, wt = [0], [], []
    for e, p in enumerate(pts):
        q = index_coords(p, origin, spacing)
        near = np.rint(q)
        q = np.where(np.abs(q - near) <= snap, near, q)
        base = np.floor(q).astype(np.int64)
        fr = q - base
        for di in (0, 1):
            for dj in (0, 1):
                for dk in (0, 1):
                    w = (fr[0] if di else 1 - fr[0]) * (fr[1] if dj else 1 - fr[1]) * (fr[2] if dk else 1 - fr[2])
                    if w == 0:
                        continue
                    v = base + (di, dj, dk)
                    if np.any(v < 0) or np.any(v >= np.asarray(n)):
                        raise ValueError(f"element {e} at {tuple(p)} m does not lie inside the grid")
                    ijk.append(v); wt.append(w)
        row.append(len(wt))
    return np.asarray(row, dtype=np.int32), np.asarray(ijk, dtype=np.int64).reshape(-1, 3), np.asarray(wt, dtype=np.float64)


def sample(T, table):
    """sum_q w_q T(vox_q) per point, accumulated in table order"""
    row, ijk, wt = table
    out = np.zeros(len(row) - 1)
    for r in range(len(row) - 1):
        acc = 0.0
        for e in range(row[r], row[r + 1]):
            acc += wt[e] * float(T[tuple(ijk[e])])
        out[r] = acc
    return out


def method(pos_m, focus_m, sound_speed, origin, spacing, c_ref, init_radius=3.0, max_sweeps=None):
    """The Eikonal method for one focus -> dict(delays [N], tau, extra_path, raw (tau from T_med alone), T_med, T_ref, sweeps)."""
    pos = np.asarray(pos_m, dtype=np.float64).reshape(-1, 3)
    focus = np.asarray(focus_m, dtype=np.float64)
    n = np.shape(sound_speed)
    table = trilinear_table(pos, origin, spacing, n)
    T_med, k_med = solve(n, origin, spacing, sound_speed, focus, init_radius, max_sweeps)
    T_ref, k_ref = solve(n, origin, spacing, float(c_ref), focus, init_radius, max_sweeps)
    t_med, t_ref = sample(T_med, table), sample(T_ref, table)
    E = c_ref * (t_med - t_ref)
    tau = np.linalg.norm(pos - focus, axis=1) / c_ref + E / c_ref
    return dict(delays=tau.max() - tau, tau=tau, extra_path=E, raw=t_med, T_med=T_med, T_ref=T_ref, sweeps=(k_med, k_ref))


# ---- scene A of the method's record: a flat fast slab between the array and the focus, against the exact Snell time -----------------
def snell_time(dx, layers):
    """Exact travel time over the lateral offset dx [m] through flat layers [(thickness m, speed m/s)]: Fermat's ray, the ray parameter p
    (sin theta_i / c_i) found by bisection on sum_i d_i p c_i / sqrt(1 - p^2 c_i^2) = dx."""
    dx = abs(float(dx))
    d = np.array([l[0] for l in layers], dtype=np.float64)
    c = np.array([l[1] for l in layers], dtype=np.float64)
    if dx == 0:
        return float(np.sum(d / c))
    lo, hi = 0.0, 1.0 / c.max()
    for _ in range(200):
        p = 0.5 * (lo + hi)
        x = np.sum(d * p * c / np.sqrt(1.0 - (p * c) ** 2))
        lo, hi = (p, hi) if x < dx else (lo, p)
    p = 0.5 * (lo + hi)
    return float(np.sum(d / (c * np.sqrt(1.0 - (p * c) ** 2))))


def scene_a(h, half_x=14e-3, half_y=4e-3, z_lo=-1e-3, z_hi=27e-3, slab=(5e-3, 9e-3), focus=(0.0, 0.0, 24e-3), el_x=12e-3, el_step=3e-3,
            c_water=1500.0, c_slab=2800.0):
    """dict(n, origin, spacing, c [n] float32, pos [E, 3], focus, layers per element for ``snell_time``): water with a flat slab on the voxel
    planes slab[0] <= z < slab[1]; elements at x = -el_x ... el_x in steps of el_step plus 0.13 mm, y = 0.15 mm, z = 0.1 mm."""
    nx, ny = 2 * int(round(half_x / h)) + 1, 2 * int(round(half_y / h)) + 1
    k_lo, k_hi = int(np.floor(z_lo / h)), int(np.ceil(z_hi / h))
    nz = k_hi - k_lo + 1
    origin = np.array([-(nx // 2) * h, -(ny // 2) * h, k_lo * h])
    z = origin[2] + np.arange(nz) * h
    in_slab = (z >= slab[0] - 1e-12) & (z < slab[1] - 1e-12)
    c = np.full((nx, ny, nz), c_water, dtype=np.float32)
    c[:, :, in_slab] = c_slab
    xs = np.arange(-el_x, el_x + 1e-9, el_step) + 0.13e-3
    pos = np.array([[x, 0.15e-3, 0.1e-3] for x in xs])
    focus = np.asarray(focus, dtype=np.float64)
    thick = int(in_slab.sum()) * h               # the voxelised slab: planes x h
    depth = focus[2] - pos[0, 2]
    layers = [(depth - thick, c_water), (thick, c_slab)]
    return dict(n=(nx, ny, nz), origin=origin, spacing=(h, h, h), c=c, pos=pos, focus=focus, layers=layers, c_ref=c_water)


def relative_error_cycles(tau, tau_ref, centre, freq):
    """Largest |(tau - tau[centre]) - (ref - ref[centre])| over the array, in cycles"""
    tau, tau_ref = np.asarray(tau), np.asarray(tau_ref)
    return float(np.abs((tau - tau[centre]) - (tau_ref - tau_ref[centre])).max() * freq)
