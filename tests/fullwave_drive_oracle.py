"""fp64 oracle of the full-wave model's drives (DESIGN.md section 2 "full-wave model: drives"), written from the definition.  NumPy only;
shares nothing with the product.

The bare drive of element e at step n (n may be negative: the same expression, the integer formed first) is
    s0_e(n) = A_e env(u) sin(2 pi frac(f0 u)),  u = (n - 1/2) dt - tau_e,  exactly 0.0 outside 0 <= u < T = cycles / f0,
and with the drive taps g_c[0 .. M_c) of e's class c on the dt grid the drive is
    s_e(n) = sum_{m = 0}^{M_c - 1} g_c[m] s0_e(n - m)      (m ascending, starting from 0.0).
A tap shifts the burst by whole steps, and the scheme is linear and invariant under whole-step shifts: ``expand`` turns every source entry
(amp, tau) of element e into the entries (amp g[m], tau + m dt), which tests/fullwave_oracle.py, the split-layer oracle and the lock-in
oracle then take unchanged; ``fir`` is the same identity on a trace."""
import numpy as np


def bare(n, A, tau, freq, cycles, ramp_cycles, dt):
    """s0(n) for an integer array ``n`` (any sign) of one element -> float64 array"""
    n = np.asarray(n, dtype=np.int64)
    T, Tr = cycles / freq, ramp_cycles / freq
    u = (n.astype(np.float64) - 0.5) * dt - tau
    ph = freq * u
    ph = ph - np.floor(ph)
    env = np.ones(u.shape)
    if Tr > 0:
        env = np.where(u < Tr, env * (0.5 * (1.0 - np.cos(np.pi * u / Tr))), env)
        env = np.where(T - u < Tr, env * (0.5 * (1.0 - np.cos(np.pi * (T - u) / Tr))), env)
    return np.where((u >= 0.0) & (u < T), A * env * np.sin(2.0 * np.pi * ph), 0.0)


def drive_table(A, tau, cls, taps, freq, cycles, ramp_cycles, dt, n_steps):
    """s[n_steps, n_el]: the drive of every (step, element); ``cls`` [n_el] class of each element, ``taps`` one 1-D array per class"""
    out = np.zeros((n_steps, len(A)))
    for e in range(len(A)):
        g = np.asarray(taps[cls[e]], dtype=np.float64)
        lead = len(g) - 1
        s0 = bare(np.arange(-lead, n_steps), A[e], tau[e], freq, cycles, ramp_cycles, dt)
        acc = np.zeros(n_steps)
        for m in range(len(g)):
            acc = acc + g[m] * s0[lead - m: lead - m + n_steps]
        out[:, e] = acc
    return out


def expand(entries, cls, taps, dt):
    """entries = (ijk [S, 3], amp [S], tau [S], element [S]) -> (ijk, amp g[m], tau + m dt) with the taps of each entry's element, entry by
    entry, m ascending"""
    ijk, amp, tau, el = entries
    o_ijk, o_amp, o_tau = [], [], []
    for q in range(len(amp)):
        g = np.asarray(taps[cls[el[q]]], dtype=np.float64)
        for m in range(len(g)):
            o_ijk.append(ijk[q]); o_amp.append(amp[q] * g[m]); o_tau.append(tau[q] + m * dt)
    return np.asarray(o_ijk, dtype=np.int64).reshape(-1, 3), np.asarray(o_amp), np.asarray(o_tau)


def fir(trace, g):
    """out[n] = sum_m g[m] trace[n - m] along axis 0 (trace[n < 0] = 0), fp64"""
    trace = np.asarray(trace, dtype=np.float64)
    out = np.zeros(trace.shape)
    for m in range(len(g)):
        out[m:] = out[m:] + g[m] * trace[:trace.shape[0] - m]
    return out


def gain(g, freq, dt):
    """G = sum_m g[m] exp(-j 2 pi f0 m dt): in the steady state the response multiplies the amplitude by |G| and shifts the lag behind
    sin(2 pi f0 t) by -arg G / 2 pi cycles"""
    g = np.asarray(g, dtype=np.float64)
    return complex(np.sum(g * np.exp(-2j * np.pi * freq * dt * np.arange(len(g)))))
