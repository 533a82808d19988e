"""Plain NumPy restatement of the analysis scans (plan/solution_analysis.py: get_mask, find_centroid, interp_transformed_axis, get_beam_bounds;
plan/solution.py: scale, analyze; plan/protocol.py: the aggregation over foci) for tests/test_gpu_scan_matrix.py.  No GPU, no kernel code: the
OPERATIONS are restated, on the grid, the per-focus 3 x 4 frame A (first three rows of inv(get_focus_matrix)), the aspect, the radii, zmin and the ops.

Per voxel  x = o + i h,  q = (A . [x, y, z, 1]) / aspect,  d = |q|  in np.longdouble (plain fp64 where that is no wider).  A voxel is IN (d < r), OUT
(d > r) or AMB(iguous): |d - r| <= 1e-9 r -- the fp64 device arithmetic may contract to FMAs and differ from this one by an ulp, so an ambiguous voxel
belongs to no mask and never carries a value.  A z plane is ambiguous against zmin when |z - zmin| <= 1e-9 hz.  `exact=True` is for dyadic grids
(origin, focus: multiples of the spacing 2^-10 m, A = [I | -focus], aspect 1): every product and sum is exact in fp64 with or without FMA, so voxels
classify by exact comparison, d == r is ON the surface ('<=' and '>=' select it, '<' and '>' do not) and nothing is ambiguous.

Volume builders take such a classification and return volumes whose scan result depends on single voxel decisions: graded_out, one_hot; tuned_radius
moves a radius next to a chosen voxel."""
import numpy as np

LD = np.longdouble
IN, OUT, AMB, ON = 1, -1, 0, 2
AMB_REL = 1e-9
OPS = ("<", "<=", ">", ">=", None)


# ---- geometry and classification --------------------------------------------------------------------------------------------------------------------
def axes(origin, spacing, n, dtype=LD):
    return [dtype(o) + np.arange(k).astype(dtype) * dtype(h) for o, h, k in zip(origin, spacing, n)]


def distance(origin, spacing, n, A, aspect):
    """d [nx, ny, nz] (longdouble) of every voxel in the focal frame A (12 numbers, row-major 3 x 4)."""
    X, Y, Z = np.meshgrid(*axes(origin, spacing, n), indexing="ij")
    A = np.asarray(A, dtype=LD).reshape(3, 4)
    q = [(A[r, 0] * X + A[r, 1] * Y + A[r, 2] * Z + A[r, 3]) / LD(aspect[r]) for r in range(3)]
    return np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2])


def classify(d, r, exact=False):
    r = LD(r)
    c = np.where(d < r, IN, OUT).astype(np.int8)
    if exact:
        c[d == r] = ON
    else:
        c[np.abs(d - r) <= LD(AMB_REL) * r] = AMB
    return c


def classify_z(oz, hz, nz, zmin, exact=False):
    """Per plane: IN = z > zmin (selected), OUT = not, AMB.  zmin None: every plane is IN."""
    if zmin is None:
        return np.full(nz, IN, dtype=np.int8)
    z = axes([oz], [hz], [nz])[0]
    c = np.where(z > LD(zmin), IN, OUT).astype(np.int8)
    if not exact:
        c[np.abs(z - LD(zmin)) <= LD(AMB_REL) * LD(hz)] = AMB
    return c


def select(cls, op):
    """Boolean mask of the voxels `dist OP r` selects; ambiguous voxels are in no mask."""
    if op is None:
        return np.ones(cls.shape, dtype=bool)
    return {"<": cls == IN, "<=": (cls == IN) | (cls == ON), ">": cls == OUT, ">=": (cls == OUT) | (cls == ON)}[op]


def bounding_box(mask):
    """[x0, x1, y0, y1, z0, z1] (half-open) of a mask: what an index box must contain.  Empty mask: an empty box."""
    if not mask.any():
        return [0, 0, 0, 0, 0, 0]
    idx = np.nonzero(mask)
    return [v for a in range(3) for v in (int(idx[a].min()), int(idx[a].max()) + 1)]


def in_box(shape, box):
    m = np.zeros(shape, dtype=bool)
    m[box[0]:box[1], box[2]:box[3], box[4]:box[5]] = True
    return m


def tuned_radius(d_voxel, side):
    """A radius that puts the voxel at distance d_voxel just inside ("in") or just outside ("out"): 1e-8 relative, far inside the fp32 pre-test's
    band (~1e-5) and ten times outside the ambiguous band."""
    return float(LD(d_voxel) * (LD(1) + LD(1e-8 if side == "in" else -1e-8)))


# ---- volume builders --------------------------------------------------------------------------------------------------------------------------------
def graded_out(mask, amb, near):
    """Zero on `mask` and on ambiguous voxels; elsewhere the distinct values N, N - 1, .. 1 (exact in fp32), the largest on the voxel with the
    smallest `near` (distance to the mask surface).  A scan over `mask` returns exactly 0, and a wrongly included voxel is named by its value."""
    vol = np.zeros(mask.shape, dtype=np.float32)
    idx = np.flatnonzero(~(mask | amb))
    order = idx[np.argsort(np.asarray(near, dtype=np.float64).ravel()[idx], kind="stable")]
    vol.ravel()[order] = np.arange(len(order), 0, -1, dtype=np.float32)
    return vol


def one_hot(mask, near, K, base=1000.0):
    """(stack [S, nx, ny, nz], flat voxel indices [S], values [S]): one spike per volume, on the K in-mask voxels nearest the surface and on the
    mask's extreme voxels along -x, +x, -y, +y, -z, +z.  The scan of volume k over `mask` returns values[k]."""
    idx = np.flatnonzero(mask)
    if idx.size == 0:
        return np.zeros((0,) + mask.shape, dtype=np.float32), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.float32)
    chosen = list(idx[np.argsort(np.asarray(near, dtype=np.float64).ravel()[idx], kind="stable")][:K])
    coords = np.unravel_index(idx, mask.shape)
    for a in range(3):
        for pick in (np.argmin, np.argmax):
            v = idx[pick(coords[a])]
            if v not in chosen:
                chosen.append(v)
    values = (base + np.arange(len(chosen))).astype(np.float32)
    stack = np.zeros((len(chosen),) + mask.shape, dtype=np.float32)
    stack.reshape(len(chosen), -1)[np.arange(len(chosen)), chosen] = values
    return stack, np.asarray(chosen, dtype=np.int64), values


# ---- the scans ----------------------------------------------------------------------------------------------------------------------------------------
def masked_peak(vol, mask):
    return np.float32(vol[mask].max()) if mask.any() else np.float32(0)


def six_peaks(p, i, main, side, zok):
    """(main p, main I, side p, side I, global p, global I): `main` carries no z test, `side` and global do (zok: [nz] or a volume mask)."""
    zm = np.broadcast_to(zok, p.shape)
    return np.array([masked_peak(v, m) for m in (main, side & zm, zm) for v in (p, i)], dtype=np.float32)


def moments(vol, mask, cut, origin, spacing):
    """(S0, Sx, Sy, Sz) over mask & (vol > cut) in fp64 (exactly rounded sums of the fp64 terms), and the gate 4 N 2^-53 sum|term| of each."""
    import math
    sel = mask & (vol > np.float32(cut))
    X, Y, Z = np.meshgrid(*axes(origin, spacing, vol.shape, dtype=np.float64), indexing="ij")
    p = vol[sel].astype(np.float64)
    terms = [p, p * X[sel], p * Y[sel], p * Z[sel]]
    N = int(sel.sum())
    return (np.array([math.fsum(t) for t in terms]), np.array([4.0 * N * 2.0 ** -53 * math.fsum(np.abs(t)) for t in terms]))


def weighted(i_stack, w):
    """max_f fl32(w_f I_f), from 0."""
    out = np.zeros(i_stack.shape[1:], dtype=np.float32)
    for f in range(i_stack.shape[0]):
        out = np.maximum(out, np.float32(w[f]) * i_stack[f])
    return out


def aggregate(p_stack, i_stack=None, denominator=None):
    """(max_f |p_f| from 0, fp64 mean_f I_f)."""
    pm = np.maximum(p_stack.max(axis=0), np.float32(0))
    if i_stack is None:
        return pm, None
    return pm, i_stack.astype(np.float64).sum(axis=0) / (denominator or i_stack.shape[0])


def scale_p(p, s):
    """Scaled |p|: one rounding of the fp64 product with the fp32 factor."""
    s = np.asarray(s, dtype=np.float32).astype(np.float64).reshape((-1,) + (1,) * (p.ndim - 1))
    return (p.astype(np.float64) * s).astype(np.float32)


def scale_i64(i, s):
    """Scaled intensity in fp64: I s^2 with the fp32 factor s (exact product of three fp32 numbers up to 2^-53)."""
    s = np.asarray(s, dtype=np.float32).astype(np.float64).reshape((-1,) + (1,) * (i.ndim - 1))
    return i.astype(np.float64) * (s * s)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


def trilinear(vol, origin, spacing, pts, tol=1e-9):
    """fp64 linear interpolation on the regular grid at pts [P, 3]; NaN outside.  A coordinate within tol (n - 1) voxels outside a face counts as
    on the face (the axis vectors of the reference are floating-point linspaces: its own end points may lie an ulp outside)."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    n = vol.shape
    inside = np.ones(len(pts), dtype=bool)
    i0, w = [], []
    for a in range(3):
        c = (pts[:, a] - origin[a]) / spacing[a]
        t = tol * max(n[a] - 1, 1)
        inside &= (c >= -t) & (c <= n[a] - 1 + t)
        cc = np.clip(np.nan_to_num(c), 0.0, n[a] - 1)
        k = np.minimum(np.floor(cc), max(n[a] - 2, 0)).astype(np.int64)
        i0.append(k); w.append(cc - k)
    acc = np.zeros(len(pts))
    v = vol.astype(np.float64)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                ww = (w[0] if dx else 1 - w[0]) * (w[1] if dy else 1 - w[1]) * (w[2] if dz else 1 - w[2])
                acc += ww * v[np.minimum(i0[0] + dx, n[0] - 1), np.minimum(i0[1] + dy, n[1] - 1), np.minimum(i0[2] + dz, n[2] - 1)]
    acc[~inside] = np.nan
    return acc


def beam_bounds(samples, cut, n_le, i_ge):
    """(last index < n_le, first index >= i_ge) whose sample lies below cut (NaN never does); -1 = none."""
    below = np.nan_to_num(np.asarray(samples, dtype=np.float64), nan=np.inf) < np.float64(cut)
    neg = np.flatnonzero(below[:n_le]); pos = np.flatnonzero(below[i_ge:])
    return (int(neg[-1]) if neg.size else -1, int(pos[0]) + i_ge if pos.size else -1)
