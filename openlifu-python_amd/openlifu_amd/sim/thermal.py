"""``run_thermal_simulation`` -- temperature rise and thermal dose of a Solution over its pulse sequence (HIP kernel 3).

An extension with no reference seam: the reference builds ``specific_heat`` and ``thermal_conductivity`` volumes but never
reads them.  The model (DESIGN.md section 2 "thermal model", kernel section 5.8, fp64 oracle tests/thermal_oracle.py):

  * Pennes bioheat equation for the rise dT above a baseline T_b:  rho Cp d(dT)/dt = div(kappa grad dT) - W dT + Q(v, t),
    Q = 2 alpha(v) 1e4 I_f(v) while a pulse aimed at focus f is on [W/m^3]; alpha = ``attenuation`` in Np/m at the pulse frequency
    (``field._np_per_m``, alpha_power 0.9), ALL of it treated as absorption (conservative).
  * explicit FTCS on ``params.coords``: 7-point stencil, face conductance = harmonic mean of kappa / h^2, dT = 0 one spacing outside
    the grid (boundary face kappa_v / h^2); the source of step n is exact in energy (the on-time of each focus' pulses inside the step).
  * outputs per voxel: the maximum rise, T_b + that, and CEM43 = sum_n dt / 60 R^(43 - T) [min].

``thermal_time_axis`` and ``thermal_schedule`` are the host halves; every refusal is raised before any device call."""
from __future__ import annotations

import numpy as np

from ..engine import get_engine, grid_from_coords
from ..util import dataset as ds
from .field import _np_per_m

_ATTRS = {"temperature_max": {"units": "degC", "long_name": "Maximum temperature"},
          "temperature_rise_max": {"units": "K", "long_name": "Maximum temperature rise"},
          "CEM43": {"units": "min", "long_name": "Cumulative equivalent minutes at 43 degC"}}
_MEDIUM_KEYS = ("density", "specific_heat", "thermal_conductivity", "attenuation")


def _axis_face_sum(kappa, axis, n_axis):
    """sum of the two face conductances along ``axis`` per voxel [W/m/K]: harmonic means inside, kappa_v on a boundary face."""
    k = np.moveaxis(kappa, axis, 0)
    out = np.empty_like(k)
    if n_axis == 1:
        out[...] = 2.0 * k
    else:
        face = 2.0 * k[1:] * k[:-1] / (k[1:] + k[:-1])
        out[...] = 0.0
        out[:-1] += face
        out[1:] += face
        out[0] += k[0]
        out[-1] += k[-1]
    return np.moveaxis(out, 0, axis)


def thermal_bound(spacing_m, n, density, specific_heat, conductivity, perfusion: float = 0.0) -> float:
    """FTCS bound dt_max = 1 / max_v (sum_faces K_face / h^2 + W) / (rho Cp)_v [s] (fp64); the medium arguments are floats or
    [nx, ny, nz] volumes, ``spacing_m`` may differ per axis."""
    h = np.broadcast_to(np.asarray(spacing_m, dtype=np.float64), (3,))
    n = tuple(int(v) for v in n)
    rc = np.asarray(density, dtype=np.float64) * np.asarray(specific_heat, dtype=np.float64)
    kap = np.asarray(conductivity, dtype=np.float64)
    if kap.ndim == 0:
        face = 2.0 * float(kap) * float(np.sum(1.0 / h ** 2))
    else:
        kap = np.broadcast_to(kap, n)
        face = sum(_axis_face_sum(kap, a, n[a]) / h[a] ** 2 for a in range(3))
    return float(1.0 / np.max((face + float(perfusion)) / rc))


def thermal_time_axis(spacing_m, n, density, specific_heat, conductivity, duration: float, dt: float = 0.0, t_end: float = 0.0,
                      perfusion: float = 0.0):
    """(dt [s], n_steps, dt_max [s]).  ``dt = 0`` gives dt_max / 2, a dt above dt_max raises ValueError; ``t_end = 0`` gives the
    sequence ``duration``; n_steps = ceil(t_end / dt) and dt shrinks to t_end / n_steps."""
    dt, t_end, perfusion, duration = float(dt), float(t_end), float(perfusion), float(duration)
    if not (np.isfinite(dt) and dt >= 0):
        raise ValueError(f"thermal simulation: dt must be finite and >= 0 (0 = default), got {dt}")
    if not (np.isfinite(t_end) and t_end >= 0):
        raise ValueError(f"thermal simulation: t_end must be finite and >= 0 (0 = the sequence duration), got {t_end}")
    if not (np.isfinite(perfusion) and perfusion >= 0):
        raise ValueError(f"thermal simulation: perfusion must be finite and >= 0, got {perfusion}")
    dt_max = thermal_bound(spacing_m, n, density, specific_heat, conductivity, perfusion)
    if dt > dt_max:
        raise ValueError(f"thermal simulation: dt = {dt:g} s is above the FTCS stability bound {dt_max:g} s")
    if dt == 0:
        dt = dt_max / 2
    if t_end == 0:
        t_end = duration
    if not t_end > 0:
        raise ValueError("thermal simulation: the sequence has no duration and no t_end was given")
    n_steps = max(1, int(np.ceil(t_end / dt * (1 - 1e-12))))
    if n_steps >= 2 ** 31:
        raise ValueError(f"thermal simulation: {n_steps} steps is too many")
    return t_end / n_steps, n_steps, dt_max


def pulse_times(pulse, sequence, n_foci: int):
    """(start [s], length [s], focus) of every pulse of the sequence: train j starts at j P (P = pulse_train_interval, or
    pulse_count pulse_interval when that is 0), pulse k of a train k pulse_interval later, lasts min(duration, pulse_interval) and
    goes to focus (k - 1) mod F (the assignment of get_ita's pulse_seq)."""
    s = sequence
    period = float(s.pulse_train_interval) or float(s.pulse_count) * float(s.pulse_interval)
    j, k = np.meshgrid(np.arange(int(s.pulse_train_count)), np.arange(int(s.pulse_count)), indexing="ij")
    start = (j * period + k * float(s.pulse_interval)).ravel()
    length = np.full(start.shape, min(float(pulse.duration), float(s.pulse_interval)))
    focus = ((k - 1) % int(n_foci)).ravel()
    return start, length, focus


def thermal_schedule(pulse, sequence, n_foci: int, dt: float, n_steps: int):
    """CSR source schedule (row_ptr [n_steps + 1] int32, focus int32, tau float64 [s]): row n lists the foci heated during
    [n dt, (n + 1) dt) with the on-time of their pulses inside it (pulses straddling a step boundary are split; time after
    n_steps dt is dropped)."""
    dt, n_steps, F = float(dt), int(n_steps), int(n_foci)
    if F < 1:
        raise ValueError("thermal simulation: the solution has no foci")
    start, length, focus = pulse_times(pulse, sequence, F)
    horizon = n_steps * dt
    end = np.minimum(start + length, horizon)
    length = np.where(end < start + length, end - start, length)       # (the exact length unless the run ends inside the pulse)
    keep = (start < horizon) & (length > 0)
    start, end, length, focus = start[keep], end[keep], length[keep], focus[keep]
    s0 = np.minimum(np.floor(start / dt).astype(np.int64), n_steps - 1)
    s1 = np.maximum(np.minimum(np.ceil(end / dt).astype(np.int64), n_steps), s0 + 1)
    cnt = s1 - s0
    # pieces: the whole pulse inside one step, else (s0 + 1) dt - start, dt ..., and the rest -- so that they sum to the length
    first = np.where(cnt == 1, length, np.minimum((s0 + 1) * dt - start, length))
    last = length - first - np.maximum(cnt - 2, 0) * dt
    idx = np.repeat(np.arange(start.size), cnt)
    pos = np.arange(idx.size) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    step = s0[idx] + pos
    tau = np.where(pos == 0, first[idx], np.where(pos == cnt[idx] - 1, last[idx], dt))
    ok = tau > 0
    step, foc, tau = step[ok], focus[idx][ok], tau[ok]
    key = step * F + foc
    uniq, inv = np.unique(key, return_inverse=True)
    tau_sum = np.bincount(inv, weights=tau, minlength=uniq.size)
    rows = uniq // F
    row_ptr = np.zeros(n_steps + 1, dtype=np.int32)
    np.add.at(row_ptr, rows + 1, 1)
    return np.cumsum(row_ptr).astype(np.int32), (uniq % F).astype(np.int32), tau_sum.astype(np.float64)


def _medium_value(params, key):
    """float for a uniform volume (declared, or constant), else the float64 volume."""
    da = params[key]
    declared = getattr(da, "uniform_value", None)
    if declared is not None:
        return float(declared)
    vol = np.asarray(da.data, dtype=np.float64)
    lo, hi = vol.min(), vol.max()
    return float(lo) if lo == hi else vol


def _coords_match(a, b) -> bool:
    da = list(a.dims) if hasattr(a, "dims") else list(a.keys())
    db = list(b.dims) if hasattr(b, "dims") else list(b.keys())
    if da != db:
        return False
    for d in da:
        va, vb = np.asarray(getattr(a[d], "data", a[d]), dtype=np.float64), np.asarray(getattr(b[d], "data", b[d]), dtype=np.float64)
        if va.shape != vb.shape or not np.array_equal(va, vb):
            return False
        if getattr(a[d], "attrs", {}).get("units") != getattr(b[d], "attrs", {}).get("units"):
            return False
    return True


def _trace_voxels(record_points, coords, n):
    """[P, 3] points in the coordinates' units -> (linear C-order voxel indices, [P, 3] voxel indices): nearest voxel."""
    dims = list(coords.dims) if hasattr(coords, "dims") else list(coords.keys())
    pts = np.atleast_2d(np.asarray(record_points, dtype=np.float64))
    if pts.shape[1] != 3:
        raise ValueError(f"record_points must be [P, 3], got {pts.shape}")
    ijk = np.empty(pts.shape, dtype=np.int64)
    for a, d in enumerate(dims):
        v = np.asarray(getattr(coords[d], "data", coords[d]), dtype=np.float64)
        h = (v[-1] - v[0]) / (len(v) - 1) if len(v) > 1 else 1.0
        i = np.rint((pts[:, a] - v[0]) / h).astype(np.int64)
        if np.any(i < 0) or np.any(i >= len(v)):
            raise ValueError("record_points: a point lies outside the grid")
        ijk[:, a] = i
    return (ijk[:, 0] * n[1] + ijk[:, 1]) * n[2] + ijk[:, 2], ijk


def run_thermal_simulation(params, solution, dt: float = 0.0, t_end: float = 0.0, baseline_temperature: float = 37.0,
                           perfusion: float = 0.0, record_points=None, pulse_energy=None):
    """Temperature rise of ``solution``'s sequence in the medium ``params`` -> (Dataset{temperature_max [degC],
    temperature_rise_max [K], CEM43 [min]} on ``params.coords``, raw{dt, n_steps, dt_max, t, traces, points_index}).

    ``dt = 0``: half the FTCS bound (a larger dt raises ValueError); ``t_end = 0``: the sequence duration (larger adds cool-down);
    ``perfusion`` W [W/m^3/K] is uniform; ``record_points`` [P, 3] in the coordinates' units are snapped to the nearest voxel and
    traced (one value of T per step).  The intensity is the Solution's (scaled if scaled), read in place while the device still holds it.
    ``pulse_energy`` [F, nx, ny, nz] in J/cm^2 on ``params.coords`` -- the pulsed model's pulse intensity integral, times factor^2 when the
    solution was scaled by ``factor`` -- replaces it: focus f then heats with ``pulse_energy[f] / min(duration, pulse_interval)``, so every
    pulse deposits exactly that energy instead of the continuous-wave estimate I min(duration, pulse_interval).  ``pulse_energy="solution"``
    takes the Solution's own "pulse_intensity_integral" (``SimSetup.options["pulse_intensity_integral"]``): read in place while the device
    still holds it (raw["source"] = "pulse_energy_resident"), else from the host variable as an array would be."""
    missing = [k for k in _MEDIUM_KEYS if k not in params]
    if missing:
        raise ValueError(f"thermal simulation: params lacks {missing}")
    res = solution.simulation_result
    if res is None or "intensity" not in res:
        raise ValueError("thermal simulation: the solution has no simulated intensity")
    inten = res["intensity"]
    F = solution.num_foci()
    coords = params.coords
    icoords = {d: inten.coords[d] for d in inten.dims if d != "focal_point_index"}
    if not _coords_match(coords, icoords):
        raise ValueError("thermal simulation: the solution's intensity is not on params.coords")
    n_vol = int(inten.shape[0])
    if n_vol != F or getattr(solution, "_sharded", False):
        raise NotImplementedError(f"thermal simulation: multi-GPU / sharded solutions are not implemented "
                                  f"(the solution holds {n_vol} of its {F} focus volumes)")
    origin, spacing, n = grid_from_coords(coords)
    source = None
    pii_resident = False
    if isinstance(pulse_energy, str):      # "solution": the Solution's own pulse intensity integral (scaled if scaled)
        if pulse_energy != "solution":
            raise ValueError(f'thermal simulation: pulse_energy must be an array or "solution", got {pulse_energy!r}')
        pii = solution._require_pii()
        pii_resident = solution._pii_on_device()
        if not pii_resident:
            pulse_energy = np.asarray(pii.data)
    if pii_resident:
        on_time = min(float(solution.pulse.duration), float(solution.sequence.pulse_interval))
        if not on_time > 0:
            raise ValueError("thermal simulation: pulse_energy needs a pulse of non-zero length")
    elif pulse_energy is not None:
        energy = np.asarray(pulse_energy, dtype=np.float64)
        if energy.shape != (F,) + tuple(int(v) for v in n):
            raise ValueError(f"thermal simulation: pulse_energy must have shape {(F,) + tuple(int(v) for v in n)}, got {energy.shape}")
        if not np.all(np.isfinite(energy)) or np.any(energy < 0):
            raise ValueError("thermal simulation: pulse_energy must be finite and >= 0 everywhere")
        on_time = min(float(solution.pulse.duration), float(solution.sequence.pulse_interval))     # (the pulse length of pulse_times)
        if not on_time > 0:
            raise ValueError("thermal simulation: pulse_energy needs a pulse of non-zero length")
        source = (energy / on_time).astype(np.float32)
    rho, cp, kap = (_medium_value(params, k) for k in ("density", "specific_heat", "thermal_conductivity"))
    att = _medium_value(params, "attenuation")
    alpha = np.asarray(att, dtype=np.float64) * _np_per_m(1.0, solution.pulse.frequency)
    alpha = float(alpha) if alpha.ndim == 0 else alpha
    dt, n_steps, dt_max = thermal_time_axis(spacing, n, rho, cp, kap, solution.sequence.get_sequence_duration(), dt, t_end, perfusion)
    row_ptr, focus, tau = thermal_schedule(solution.pulse, solution.sequence, F, dt, n_steps)
    pts, ijk = (np.zeros(0, dtype=np.int64), np.zeros((0, 3), dtype=np.int64)) if record_points is None else _trace_voxels(record_points, coords, n)
    eng = get_engine()
    if getattr(eng.ctx, "nranks", 1) > 1:
        raise NotImplementedError("thermal simulation: multi-GPU is not implemented (the context belongs to a communicator)")
    if pii_resident:      # read in place [J/cm^2]: 1 / (pulse on-time) goes into the on-times of the schedule instead of into the volumes
        tau = tau / on_time
    resident = source is None and not pii_resident and solution._device_is_current()
    if source is None and not resident and not pii_resident:
        source = np.asarray(inten.data)
    rise, cem, traces = eng.thermal(origin, spacing, n, (rho, cp, kap, alpha), float(perfusion), (row_ptr, focus, tau), F,
                                    dt, float(baseline_temperature), source, pts, pii_source=pii_resident)
    dims = list(coords.dims) if hasattr(coords, "dims") else list(coords.keys())
    tmax = (float(baseline_temperature) + rise.astype(np.float64)).astype(np.float32)
    out = {name: ds.make_dataarray(vol, coords=coords, dims=dims, name=name, attrs=_ATTRS[name])
           for name, vol in (("temperature_max", tmax), ("temperature_rise_max", rise), ("CEM43", cem))}
    raw = {"dt": dt, "n_steps": n_steps, "dt_max": dt_max, "t": (np.arange(n_steps) + 1) * dt,
           "traces": float(baseline_temperature) + traces.astype(np.float64), "points_index": ijk,
           "source": "pulse_energy_resident" if pii_resident else "pulse_energy" if pulse_energy is not None else "resident" if resident else "uploaded", "backend": "openlifu_amd/hip-gfx950"}
    return ds.make_dataset(out), raw
