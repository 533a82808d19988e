"""fp64 NumPy restatement of the thermal model's discrete scheme (DESIGN.md section 2 "thermal model"; HIP kernel 3,
openlifu-python_amd/csrc/k_thermal.hip): explicit FTCS for the Pennes rise dT with a 7-point stencil, harmonic-mean face
conductances, dT = 0 one spacing outside the grid, the energy-exact source of a CSR schedule, and the CEM43 rule."""
import numpy as np


def face_conductances(kappa, spacing, shape, arith=False):
    """[3] arrays K+ (the face between v and v + e_a, [n_a] along axis a with the last one the boundary face) and K- (between v and
    v - e_a, the first one the boundary face), over h^2 [W/m^3/K].  ``arith``: the arithmetic mean in place of the harmonic one (a
    perturbation of ``run``, never the scheme)."""
    kap = np.broadcast_to(np.asarray(kappa, dtype=np.float64), shape)
    plus, minus = [], []
    for a in range(3):
        k = np.moveaxis(kap, a, 0)
        kp = np.empty_like(k); km = np.empty_like(k)
        if k.shape[0] > 1:
            face = 0.5 * (k[1:] + k[:-1]) if arith else 2.0 * k[1:] * k[:-1] / (k[1:] + k[:-1])
            kp[:-1] = face; km[1:] = face
        kp[-1] = k[-1]; km[0] = k[0]
        h2 = float(spacing[a]) ** 2
        plus.append(np.moveaxis(kp, 0, a) / h2); minus.append(np.moveaxis(km, 0, a) / h2)
    return plus, minus


def ftcs_bound(rho, cp, kappa, spacing, shape, perfusion=0.0):
    plus, minus = face_conductances(kappa, spacing, shape)
    rc = np.broadcast_to(np.asarray(rho, dtype=np.float64) * np.asarray(cp, dtype=np.float64), shape)
    return 1.0 / np.max((sum(plus) + sum(minus) + perfusion) / rc)


def _shift(t, a, d):
    """t at v + d e_a (d = +-1), 0 outside the grid."""
    out = np.zeros_like(t)
    src = [slice(None)] * 3; dst = [slice(None)] * 3
    if d > 0:
        src[a] = slice(1, None); dst[a] = slice(None, -1)
    else:
        src[a] = slice(None, -1); dst[a] = slice(1, None)
    out[tuple(dst)] = t[tuple(src)]
    return out


# Named perturbations of ``run``: each one is a plausible slip of a kernel of this scheme.  A parity table is sensitive to a slip when the
# perturbed oracle leaves the unperturbed one by far more than the table's gate (tests/test_gpu_thermal_matrix.py).
PERTURBATIONS = {
    "arith": "arithmetic in place of harmonic mean on the inner faces",
    "noface0+": "the boundary face at the high end of x dropped", "noface0-": "the boundary face at the low end of x dropped",
    "noface1+": "the boundary face at the high end of y dropped", "noface1-": "the boundary face at the low end of y dropped",
    "noface2+": "the boundary face at the high end of z dropped", "noface2-": "the boundary face at the low end of z dropped",
    "swapyz_minus": "the y and z conductances of the minus faces exchanged",
    "s_uniform": "the source factor of voxel 0 used everywhere",
    "noperf": "perfusion dropped",
    "rowshift": "step n heats with the schedule's row n + 1",
    "cemlag": "CEM43 reads the temperature before the step",
    "riselag": "rise_max reads dT before the step",
}


def _perturb_faces(plus, minus, pert):
    if pert is not None and pert.startswith("noface"):
        ax, side = int(pert[6]), pert[7]
        arr = (plus if side == "+" else minus)[ax]
        edge = [slice(None)] * 3
        edge[ax] = -1 if side == "+" else 0
        arr[tuple(edge)] = 0.0
    if pert == "swapyz_minus":
        minus[1], minus[2] = minus[2], minus[1]


def run(rho, cp, kappa, alpha_np_m, intensity, spacing, row_ptr, focus, tau, dt, n_steps, baseline=37.0, perfusion=0.0, points=None,
        t0=None, pert=None):
    """-> (rise_max [K], CEM43 [min], traces [n_steps, P] of dT [K], final dT).  ``intensity`` [F, nx, ny, nz] W/cm^2.
    ``pert``: None (the scheme) or a key of PERTURBATIONS (the scheme with that slip)."""
    if pert is not None and pert not in PERTURBATIONS:
        raise ValueError(f"unknown perturbation {pert!r}")
    inten = np.asarray(intensity, dtype=np.float64)
    shape = inten.shape[1:]
    plus, minus = face_conductances(kappa, spacing, shape, arith=pert == "arith")
    _perturb_faces(plus, minus, pert)
    if pert == "noperf":
        perfusion = 0.0
    rc = np.broadcast_to(np.asarray(rho, dtype=np.float64) * np.asarray(cp, dtype=np.float64), shape)
    a = 1.0 / rc
    s = 2.0 * np.broadcast_to(np.asarray(alpha_np_m, dtype=np.float64), shape) * 1e4 / rc
    if pert == "s_uniform":
        s = np.full(shape, s.ravel()[0])
    t = np.zeros(shape) if t0 is None else np.array(t0, dtype=np.float64)
    rise = np.zeros(shape)
    cem = np.zeros(shape)
    pts = np.zeros(0, dtype=np.int64) if points is None else np.asarray(points, dtype=np.int64)
    traces = np.zeros((n_steps, pts.size))
    for n in range(n_steps):
        acc = -perfusion * t
        for ax in range(3):
            acc += plus[ax] * (_shift(t, ax, +1) - t) + minus[ax] * (_shift(t, ax, -1) - t)
        q = np.zeros(shape)
        row = n + 1 if pert == "rowshift" else n
        for e in range(int(row_ptr[row]), int(row_ptr[row + 1])) if row < n_steps else ():
            q += float(tau[e]) * inten[int(focus[e])]
        before = t
        t = t + dt * a * acc + s * q
        rise = np.maximum(rise, before if pert == "riselag" else t)
        temp = baseline + (before if pert == "cemlag" else t)
        cem += dt / 60.0 * np.where(temp >= 43.0, 0.5, 0.25) ** (43.0 - temp)
        traces[n] = t.ravel()[pts]
    return rise, cem, traces, t


def run32(rho, cp, kappa, alpha_np_m, intensity, spacing, row_ptr, focus, tau, dt, n_steps, baseline=37.0, perfusion=0.0, points=None):
    """The same scheme with every stored quantity in float32, as the header comment of k_thermal.hip lays a step out (written from
    that description, not from the kernel's code): the float32 roundings of ``face_conductances``, 1/(rho Cp), s, W, the on-times, dt,
    dt/60 and T_b - 43; the state, rise_max and CEM43 in float32;
        acc = sum_+ K+ (dT_nb - dT) + sum_- K- (dT_nb - dT) - W dT,   dT' = dT + (dt / (rho Cp)) acc + s sum_f tau_f I_f,
        rise_max = max(rise_max, dT'),   cem += dt/60 2^x or 4^x,   x = (T_b - 43) + dT'   (>= 0: 2^x)
    every operation rounded to float32.  Its distance from ``run`` is the scale of the rounding no fp32 kernel of this scheme can avoid;
    a gate is set from it, never from a kernel's output.  -> (rise_max, CEM43, traces, final dT), float32."""
    f32 = np.float32
    inten = np.asarray(intensity, dtype=f32)
    shape = inten.shape[1:]
    plus, minus = face_conductances(kappa, spacing, shape)
    plus = [p.astype(f32) for p in plus]; minus = [m.astype(f32) for m in minus]
    rc = np.broadcast_to(np.asarray(rho, dtype=np.float64) * np.asarray(cp, dtype=np.float64), shape)
    a = (1.0 / rc).astype(f32)
    s = (2.0 * np.broadcast_to(np.asarray(alpha_np_m, dtype=np.float64), shape) * 1e4 / rc).astype(f32)
    w, dt32, dt_min, tb43 = f32(perfusion), f32(dt), f32(dt / 60.0), f32(baseline - 43.0)
    tau32 = np.asarray(tau, dtype=np.float64).astype(f32)
    t = np.zeros(shape, dtype=f32)
    rise = np.zeros(shape, dtype=f32)
    cem = np.zeros(shape, dtype=f32)
    pts = np.zeros(0, dtype=np.int64) if points is None else np.asarray(points, dtype=np.int64)
    traces = np.zeros((n_steps, pts.size), dtype=f32)
    for n in range(n_steps):
        acc = np.zeros(shape, dtype=f32)
        for ax in range(3):
            acc += plus[ax] * (_shift(t, ax, +1) - t)
        for ax in range(3):
            acc += minus[ax] * (_shift(t, ax, -1) - t)
        acc -= w * t
        q = np.zeros(shape, dtype=f32)
        for e in range(int(row_ptr[n]), int(row_ptr[n + 1])):
            q += tau32[e] * inten[int(focus[e])]
        t = t + (dt32 * a) * acc + s * q
        rise = np.maximum(rise, t)
        x = tb43 + t
        cem += dt_min * np.exp2(np.where(x >= 0, x, f32(2.0) * x))
        traces[n] = t.ravel()[pts]
        assert t.dtype == f32 and cem.dtype == f32 and acc.dtype == f32
    return rise, cem, traces, t


