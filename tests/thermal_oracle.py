"""fp64 NumPy restatement of the thermal model's discrete scheme (DESIGN.md section 2 "thermal model"; HIP kernel 3,
openlifu-python_amd/csrc/k_thermal.hip): explicit FTCS for the Pennes rise dT with a 7-point stencil, harmonic-mean face
conductances, dT = 0 one spacing outside the grid, the energy-exact source of a CSR schedule, and the CEM43 rule."""
import numpy as np


def face_conductances(kappa, spacing, shape):
    """[3] arrays K+ (the face between v and v + e_a, [n_a] along axis a with the last one the boundary face) and K- (between v and
    v - e_a, the first one the boundary face), over h^2 [W/m^3/K]."""
    kap = np.broadcast_to(np.asarray(kappa, dtype=np.float64), shape)
    plus, minus = [], []
    for a in range(3):
        k = np.moveaxis(kap, a, 0)
        kp = np.empty_like(k); km = np.empty_like(k)
        if k.shape[0] > 1:
            face = 2.0 * k[1:] * k[:-1] / (k[1:] + k[:-1])
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


def run(rho, cp, kappa, alpha_np_m, intensity, spacing, row_ptr, focus, tau, dt, n_steps, baseline=37.0, perfusion=0.0, points=None,
        t0=None):
    """-> (rise_max [K], CEM43 [min], traces [n_steps, P] of dT [K], final dT).  ``intensity`` [F, nx, ny, nz] W/cm^2."""
    inten = np.asarray(intensity, dtype=np.float64)
    shape = inten.shape[1:]
    plus, minus = face_conductances(kappa, spacing, shape)
    rc = np.broadcast_to(np.asarray(rho, dtype=np.float64) * np.asarray(cp, dtype=np.float64), shape)
    a = 1.0 / rc
    s = 2.0 * np.broadcast_to(np.asarray(alpha_np_m, dtype=np.float64), shape) * 1e4 / rc
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
        for e in range(int(row_ptr[n]), int(row_ptr[n + 1])):
            q += float(tau[e]) * inten[int(focus[e])]
        t = t + dt * a * acc + s * q
        rise = np.maximum(rise, t)
        temp = baseline + t
        cem += dt / 60.0 * np.where(temp >= 43.0, 0.5, 0.25) ** (43.0 - temp)
        traces[n] = t.ravel()[pts]
    return rise, cem, traces, t
