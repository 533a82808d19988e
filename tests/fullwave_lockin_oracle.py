"""fp64 oracle of the full-wave lock-in and of the TimeReversal delays (DESIGN.md section 2 "full-wave model" / "TimeReversal", kernel
section 5.15), written from the definitions.  The field itself comes from tests/fullwave_oracle.py (imported, not edited): ``simulate``
traces p~ of every step at the voxels asked for, and the sums are formed here from those traces.  Shares nothing with the product's
host helpers except inputs.

Window: the steps n in [w0, w0 + Nw); t_n = (n + 1) dt; theta_n = 2 pi frac(f0 t_n).
  volume    C(v) = sum_n p~_n(v) cosf_n, S(v) = sum_n p~_n(v) sinf_n, cosf_n / sinf_n = cos / sin theta_n rounded once to float32
  receiver  s_r(n) = sum_q w_q p~_n(vox_q) in table order; C_r = sum_n s_r(n) cos theta_n, S_r = sum_n s_r(n) sin theta_n
  outputs   A = 2 / Nw hypot(C, S); psi = atan2(-C, S) / 2 pi in (-1/2, 1/2]: the lag of p behind sin(2 pi f0 t) [cycles]
TimeReversal, from the received Z_e = C_e + i S_e and an anchor's relative delays d_e:
  x_e = -f0 d_e - psi_e; off = arg(sum_e |Z_e| exp(2 pi i x_e)) / 2 pi; m_e = rint(x_e - off); T_e = (psi_e + m_e) / f0;
  delays_e = max T - T_e; tie margin = 1/2 - max_e |x_e - off - m_e|."""
import numpy as np

import fullwave_oracle as fo


def angles(freq, dt, w0, nw):
    ph = freq * ((np.arange(w0, w0 + nw, dtype=np.float64) + 1.0) * dt)
    return 2.0 * np.pi * (ph - np.floor(ph))


def volume_sums(trace, freq, dt, w0, nw):
    """trace [n_steps, V] -> (C [V], S [V]) with the float32-rounded cosine and sine the device is handed."""
    th = angles(freq, dt, w0, nw)
    cf, sf = np.cos(th).astype(np.float32).astype(np.float64), np.sin(th).astype(np.float32).astype(np.float64)
    win = trace[w0:w0 + nw]
    return cf @ win, sf @ win


def receiver_sums(trace, column_of, row, voxels, weights, freq, dt, w0, nw):
    """trace [n_steps, V] whose column ``column_of[vox]`` is voxel ``vox``; the CSR table -> (C_r [R], S_r [R])."""
    th = angles(freq, dt, w0, nw)
    win = trace[w0:w0 + nw]
    R = len(row) - 1
    C, S = np.zeros(R), np.zeros(R)
    for r in range(R):
        s = np.zeros(nw)
        for q in range(row[r], row[r + 1]):
            s = s + weights[q] * win[:, column_of[int(voxels[q])]]
        C[r], S[r] = s @ np.cos(th), s @ np.sin(th)
    return C, S


def amplitude_phase(C, S, nw):
    psi = np.arctan2(-np.asarray(C, dtype=np.float64), np.asarray(S, dtype=np.float64)) / (2.0 * np.pi)
    return 2.0 / nw * np.hypot(C, S), np.where(psi <= -0.5, 0.5, psi)


def trilinear(points, origin, h, n, snap=1e-9):
    """CSR trilinear table of points [P, 3] m on the grid with voxel 0 at ``origin`` -> (row [P + 1], ijk [S, 3], weight [S]); weights of 0
    dropped, a coordinate within ``snap`` voxels of a voxel centre counts as on it."""
    h = np.broadcast_to(np.asarray(h, dtype=np.float64), (3,))
    row, ijk, wt = [0], [], []
    for r in np.atleast_2d(np.asarray(points, dtype=np.float64)):
        q = (r - np.asarray(origin, dtype=np.float64)) / h
        q = np.where(np.abs(q - np.rint(q)) <= snap, np.rint(q), q)
        lo = np.floor(q).astype(int)
        f = q - lo
        for corner in np.ndindex(2, 2, 2):
            w = np.prod([f[a] if corner[a] else 1.0 - f[a] for a in range(3)])
            if w == 0:
                continue
            v = lo + np.array(corner)
            assert np.all(v >= 0) and np.all(v < np.asarray(n)), (r, v)
            ijk.append(v); wt.append(w)
        row.append(len(ijk))
    return np.array(row, dtype=np.int64), np.array(ijk, dtype=np.int64).reshape(-1, 3), np.array(wt, dtype=np.float64)


def time_reversal(Z, anchor_delays, freq):
    """(delays [N] s, tie margin [cycles], m [N], psi [N])"""
    Z = np.asarray(Z, dtype=np.complex128)
    _, psi = amplitude_phase(Z.real, Z.imag, 1)
    x = -freq * np.asarray(anchor_delays, dtype=np.float64) - psi
    off = np.angle(np.sum(np.abs(Z) * np.exp(2j * np.pi * x))) / (2.0 * np.pi)
    m = np.rint(x - off)
    T = (psi + m) / freq
    return T.max() - T, float(0.5 - np.abs(x - off - m).max()), m, psi


def window_of(n_steps, dt, freq, lockin_cycles):
    nw = int(np.rint(lockin_cycles / (freq * dt)))
    return n_steps - nw, nw


def drive_cycles(freq, t_end):
    return float(np.ceil(freq * t_end) + 1.0)


def steady_receivers(n, h, c, rho, alpha, c_ref, pml, pml_alpha, dt, n_steps, src, rec_points, freq, cycles, ramp, w0, nw, origin=(0, 0, 0),
                     trace_extra=()):
    """One driven run with the sources ``src = (ijk, amp, tau)``; receivers at ``rec_points`` [P, 3] m (trilinear) -> (Z [P], trace of
    ``trace_extra`` voxels [n_steps, len(trace_extra)])."""
    row, ijk, wt = trilinear(rec_points, origin, h, n)
    extra = np.asarray(trace_extra, dtype=np.int64).reshape(-1, 3)
    allv = np.concatenate([ijk, extra]) if extra.size else ijk
    uniq, inv = np.unique(allv, axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    tr = fo.simulate(n, h, c, rho, alpha, c_ref, pml, pml_alpha, dt, n_steps, src[0], src[1], src[2], freq, cycles, ramp, trace_ijk=uniq)["trace"]
    column_of = {q: int(inv[q]) for q in range(len(ijk))}
    C, S = receiver_sums(tr, column_of, row, np.arange(len(ijk)), wt, freq, dt, w0, nw)
    return C + 1j * S, tr[:, inv[len(ijk):]]
