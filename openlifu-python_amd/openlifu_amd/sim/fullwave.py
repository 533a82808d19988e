"""``run_fullwave_simulation`` -- full-wave FDTD field model (HIP kernel 5): reflection, refraction and transmission loss at the
interfaces of a heterogeneous medium, which the ray models (kernels 2a-2ph) leave out.

An opt-in model with the reference seam's leading arguments, so it can stand in for ``run_simulation`` where
``Protocol.calc_solution`` runs a replaced seam.  The model (DESIGN.md section 2 "full-wave model", kernel
section 5.14, fp64 oracle tests/fullwave_oracle.py): linear acoustics, first order in (p, v), on a staggered grid -- second order in
time, fourth order in space -- with narrow-band absorption exp(-2 alpha c dt) per step (alpha at the drive frequency), monopole
sources spread trilinearly over the 8 voxels around each element, and absorbing layers of ``pml_size`` voxels OUTSIDE ``params.coords``
(the medium is extended by edge replication, the results are cropped back).

``fullwave_time_axis``, ``layer_profile``, ``pad_volume`` / ``crop_volume`` and ``source_table`` are the host halves (pure functions);
every refusal is raised before any device call."""
from __future__ import annotations

import logging

import numpy as np

from ..engine import Engine, get_engine, grid_from_coords
from ..util import dataset as ds
from .field import _ATTRS, _medium, _np_per_m

PPW_WARN = 8.0      # points per wavelength below which the fourth-order stencil's dispersion error is no longer small


def stability_bound(spacing_m, c_max: float) -> float:
    """dt_max = 6 / (7 c_max sqrt(sum_a 1 / h_a^2)) [s]: the von Neumann bound of the (2, 4) staggered scheme (CFL 0.495 for cubic voxels)."""
    h = np.broadcast_to(np.asarray(spacing_m, dtype=np.float64), (3,))
    return float(6.0 / (7.0 * float(c_max) * np.sqrt(np.sum(1.0 / h ** 2))))


def fullwave_time_axis(spacing_m, n, sound_speed, freq: float, cycles: float, delays=0.0, dt: float = 0.0, t_end: float = 0.0,
                       cfl: float = 0.3):
    """(dt [s], n_steps, dt_max [s], points_per_wavelength).  ``sound_speed`` is a float or a volume; ``n`` the caller's (unpadded)
    grid.  ``dt = 0`` gives min(cfl h_min / c_max, 0.9 dt_max) -- ``cfl`` is a request that never makes the run unstable -- and a dt
    above dt_max raises ValueError; ``t_end = 0`` gives |n h| / c_min + max(delays) + cycles / freq; n_steps = ceil(t_end / dt).
    points_per_wavelength = c_min / (freq h_max); below 8 a warning is logged (the run is not refused)."""
    h = np.broadcast_to(np.asarray(spacing_m, dtype=np.float64), (3,))
    n = np.asarray([int(v) for v in n], dtype=np.float64)
    cs = np.asarray(sound_speed, dtype=np.float64)
    dt, t_end, cfl, freq, cycles = float(dt), float(t_end), float(cfl), float(freq), float(cycles)
    if not (np.all(np.isfinite(h)) and np.all(h > 0)):
        raise ValueError(f"full-wave simulation: spacing must be finite and > 0, got {h}")
    if not (cs.size and np.all(np.isfinite(cs)) and np.all(cs > 0)):
        raise ValueError("full-wave simulation: sound speed must be finite and > 0 everywhere")
    if not (np.isfinite(freq) and freq > 0 and np.isfinite(cycles) and cycles > 0):
        raise ValueError(f"full-wave simulation: freq and cycles must be finite and > 0, got {freq}, {cycles}")
    if not (np.isfinite(dt) and dt >= 0 and np.isfinite(t_end) and t_end >= 0):
        raise ValueError(f"full-wave simulation: dt and t_end must be finite and >= 0 (0 = default), got dt={dt}, t_end={t_end}")
    c_max, c_min = float(cs.max()), float(cs.min())
    dt_max = stability_bound(h, c_max)
    if dt > dt_max:
        raise ValueError(f"full-wave simulation: dt = {dt:g} s is above the stability bound {dt_max:g} s")
    if dt == 0:
        if not (np.isfinite(cfl) and cfl > 0):
            raise ValueError(f"full-wave simulation: the default dt needs cfl > 0, got {cfl}")
        dt = min(cfl * float(h.min()) / c_max, 0.9 * dt_max)
    if t_end == 0:
        tau = np.asarray(delays, dtype=np.float64)
        t_end = float(np.sqrt(np.sum((n * h) ** 2))) / c_min + (float(tau.max()) if tau.size else 0.0) + cycles / freq
    n_steps = max(1, int(np.ceil(t_end / dt * (1 - 1e-12))))
    if n_steps >= 2 ** 31:
        raise ValueError(f"full-wave simulation: {n_steps} steps is too many")
    ppw = c_min / (freq * float(h.max()))
    if ppw < PPW_WARN:
        logging.getLogger(__name__).warning("full-wave simulation: %.1f points per wavelength (c_min / (freq h_max)) is below %g: "
                                            "the fourth-order stencil's dispersion error grows quickly there", ppw, PPW_WARN)
    return dt, n_steps, dt_max, ppw


def layer_profile(n_padded: int, spacing_m: float, pml_size: int, pml_alpha: float, c_ref: float, dt: float):
    """d[i], i < n_padded: the decay per step along one axis, exp(-pml_alpha (c_ref / h) (depth / pml_size)^4 dt) with depth = the
    number of voxels into the layer (1 .. pml_size from the interior outwards), 1 in the interior."""
    n_padded, pml_size = int(n_padded), int(pml_size)
    i = np.arange(n_padded)
    depth = np.maximum(np.maximum(pml_size - i, i - (n_padded - 1 - pml_size)), 0)
    x = depth / pml_size if pml_size > 0 else np.zeros(n_padded)
    return np.exp(-float(pml_alpha) * (float(c_ref) / float(spacing_m)) * x ** 4 * float(dt))


def pad_volume(vol, pml_size: int):
    """[nx, ny, nz] -> the volume extended by ``pml_size`` voxels per side by edge replication."""
    return np.pad(np.asarray(vol), int(pml_size), mode="edge")


def crop_volume(vol, pml_size: int):
    """The inverse of ``pad_volume``: the caller's grid out of a padded volume."""
    q = int(pml_size)
    return np.ascontiguousarray(vol[q:vol.shape[0] - q, q:vol.shape[1] - q, q:vol.shape[2] - q]) if q else np.asarray(vol)


def source_table(pos_m, area, apod, delays, origin_m, spacing_m, n, sound_speed, c_ref, freq, p0, dt, snap: float = 1e-9):
    """Monopole source entries on the caller's (unpadded) grid -> (ijk [S, 3] int64, amplitude [S], tau [S], element [S]).

    Element e contributes to the 8 voxels around its position with trilinear weights; weights of 0 are dropped, so an element
    exactly on a voxel gives one entry (a position within ``snap`` voxels of a voxel centre counts as on it).  amplitude =
    weight dt c(vox)^2 4 pi A_e / (2 pi freq h_x h_y h_z) with A_e = apod_e p0 area_e freq / c_ref: the monopole whose free-field
    pressure is A_e / r cos(2 pi freq (t - tau_e - r / c)).  An element with a weighted voxel outside the grid raises ValueError."""
    pos = np.atleast_2d(np.asarray(pos_m, dtype=np.float64))
    h = np.broadcast_to(np.asarray(spacing_m, dtype=np.float64), (3,))
    n = tuple(int(v) for v in n)
    cs = np.asarray(sound_speed, dtype=np.float64)
    A = np.asarray(apod, dtype=np.float64) * np.asarray(area, dtype=np.float64) * float(p0) * float(freq) / float(c_ref)
    tau = np.asarray(delays, dtype=np.float64)
    scale = float(dt) * 4.0 * np.pi / (2.0 * np.pi * float(freq) * float(np.prod(h)))
    ijk, amp, tt, el = [], [], [], []
    for e in range(pos.shape[0]):
        q = (pos[e] - np.asarray(origin_m, dtype=np.float64)) / h
        near = np.rint(q)
        q = np.where(np.abs(q - near) <= snap, near, q)
        base = np.floor(q).astype(np.int64)
        frac = q - base
        for di in (0, 1):
            for dj in (0, 1):
                for dk in (0, 1):
                    w = (frac[0] if di else 1 - frac[0]) * (frac[1] if dj else 1 - frac[1]) * (frac[2] if dk else 1 - frac[2])
                    if w == 0:
                        continue
                    v = base + (di, dj, dk)
                    if np.any(v < 0) or np.any(v >= n):
                        raise ValueError(f"full-wave simulation: element {e} at {tuple(pos[e])} m does not lie inside the grid "
                                         f"(its source voxel {tuple(int(t) for t in v)} is outside {n})")
                    c_v = float(cs) if cs.ndim == 0 else float(cs[tuple(v)])
                    ijk.append(v); amp.append(w * scale * c_v * c_v * A[e]); tt.append(tau[e]); el.append(e)
    return (np.asarray(ijk, dtype=np.int64).reshape(-1, 3), np.asarray(amp, dtype=np.float64), np.asarray(tt, dtype=np.float64),
            np.asarray(el, dtype=np.int64))


def _broadcast(value, ref, shape):
    return np.full(shape, ref, dtype=np.float64) if value is None else np.asarray(value, dtype=np.float64)


def run_fullwave_simulation(arr, params, delays=None, apod=None, freq: float = 1e6, cycles: float = 20, amplitude: float = 1,
                            dt: float = 0, t_end: float = 0, cfl: float = 0.3, bli_tolerance: float = 0.05, upsampling_rate: int = 5,
                            gpu: bool = True, ref_values_only: bool = False, *, pml_size: int = 16, pml_alpha: float = 2.0,
                            ramp_cycles: float = 0.0, pulse_intensity_integral: bool = False, record_points=None):
    """Full-wave simulation of one steering -> (Dataset{p_max [Pa], p_min [Pa], intensity [W/cm^2]} on ``params.coords``, raw).

    The leading arguments are ``run_simulation``'s; ``bli_tolerance`` / ``upsampling_rate`` / ``gpu`` are accepted and ignored (there is
    no CPU path).  ``delays`` are used as given (no truncation to whole steps).  intensity = 1e-4 p_min^2 / (2 rho c) and, with
    ``pulse_intensity_integral``, PII = 1e-4 dt sum p^2 / (rho c) [J/cm^2], both with the voxel's own rho c.  ``record_points`` [P, 3] in
    the coordinates' units adds "p_trace" [P, n_steps] (p after each step), "t" and "trace_voxels" to ``raw``."""
    n_el = arr.numelements()
    delays = np.zeros(n_el) if delays is None else np.asarray(delays, dtype=np.float64)
    apod = np.ones(n_el) if apod is None else np.asarray(apod, dtype=np.float64)
    if delays.shape != (n_el,) or apod.shape != (n_el,):
        raise ValueError(f"delays and apod must have shape ({n_el},), got {delays.shape} and {apod.shape}")
    if not (np.all(np.isfinite(delays)) and np.all(np.isfinite(apod))):
        raise ValueError("full-wave simulation: delays and apod must be finite")
    pml_size = int(pml_size)
    if pml_size < 0 or not (np.isfinite(pml_alpha) and pml_alpha >= 0):
        raise ValueError(f"full-wave simulation: pml_size must be >= 0 and pml_alpha finite and >= 0, got {pml_size}, {pml_alpha}")
    if not (np.isfinite(ramp_cycles) and 0 <= ramp_cycles):
        raise ValueError(f"full-wave simulation: ramp_cycles must be finite and >= 0, got {ramp_cycles}")
    coords = params.coords
    origin, spacing, n = grid_from_coords(coords)
    n = tuple(int(v) for v in n)
    c_ref, rho_ref, medium, absorption = _medium(params, freq, ref_values_only)
    if medium is None:      # homogeneous: the uniform instantiation streams no coefficient volume
        cs, rho, alpha = c_ref, rho_ref, float(absorption)
    else:
        cs = c_ref if medium["sound_speed"] is None else np.asarray(medium["sound_speed"], dtype=np.float64)
        rho = rho_ref if medium["density"] is None else np.asarray(medium["density"], dtype=np.float64)
        alpha = 0.0 if medium["attenuation"] is None else np.asarray(medium["attenuation"], dtype=np.float64) * _np_per_m(1.0, freq)
    dt, n_steps, dt_max, ppw = fullwave_time_axis(spacing, n, cs, freq, cycles, delays, dt, t_end, cfl)
    pos, _, area, _ = Engine._table_of(arr)
    p0 = float(amplitude) * (1.0 if arr.sensitivity is None else float(arr.sensitivity))
    ijk, amp, tau, _ = source_table(pos, area, apod, delays, origin, spacing, n, cs, c_ref, freq, p0, dt)
    trace_voxels = tr_ijk = None
    if record_points is not None:
        from .thermal import _trace_voxels      # (the same nearest-voxel rule as the thermal traces)
        trace_voxels, tr_ijk = _trace_voxels(record_points, coords, n)
    npad = tuple(v + 2 * pml_size for v in n)

    def lin(v):
        v = v + pml_size
        return (v[:, 0] * npad[1] + v[:, 1]) * npad[2] + v[:, 2]

    vols = [v if np.ndim(v) == 0 else pad_volume(v, pml_size) for v in (cs, rho, alpha)]
    logging.info("Running full-wave simulation")
    eng = get_engine()
    pmax, pmin, psq, trace = eng.fullwave(spacing, npad, vols, c_ref, pml_size, pml_alpha, dt, n_steps, (lin(ijk), amp, tau), freq, cycles,
                                          ramp_cycles, psq=bool(pulse_intensity_integral), points=None if tr_ijk is None else lin(tr_ijk))
    logging.info("Simulation Complete")
    pmax, pmin = crop_volume(pmax, pml_size), crop_volume(pmin, pml_size)
    # the impedance of the intensity: the volumes' own rho c (with ref_values_only too, as run_simulation forms it)
    if ref_values_only:
        uniform = all(getattr(params[k], "uniform_value", None) is not None for k in ("density", "sound_speed"))
        Z = rho_ref * c_ref if uniform else np.asarray(params["density"].data, dtype=np.float64) * np.asarray(params["sound_speed"].data, dtype=np.float64)
    else:
        Z = np.asarray(rho, dtype=np.float64) * np.asarray(cs, dtype=np.float64)
    inten = (1e-4 * pmin.astype(np.float64) ** 2 / (2.0 * Z)).astype(np.float32)
    dims = list(coords.dims) if hasattr(coords, "dims") else list(coords.keys())
    out = {"p_max": ds.make_dataarray(pmax, coords=coords, dims=dims, name="p_max", attrs=_ATTRS["p_max"]),
           "p_min": ds.make_dataarray(pmin.copy(), coords=coords, dims=dims, name="p_min", attrs=_ATTRS["p_min"]),
           "intensity": ds.make_dataarray(inten, coords=coords, dims=dims, name="I", attrs=_ATTRS["intensity"])}
    dataset = ds.make_dataset(out)
    raw = {"p_max": pmax, "p_min": -pmin, "dt": dt, "n_steps": n_steps, "dt_max": dt_max, "points_per_wavelength": ppw,
           "backend": "openlifu_amd/hip-gfx950"}
    if pulse_intensity_integral:
        pii = (1e-4 * dt * crop_volume(psq, pml_size).astype(np.float64) / Z).astype(np.float32)
        dataset["pulse_intensity_integral"] = ds.make_dataarray(pii, coords=coords, dims=dims, name="pulse_intensity_integral",
                                                                attrs=_ATTRS["pulse_intensity_integral"])
        raw["pulse_intensity_integral"] = pii
    if trace_voxels is not None:
        raw["p_trace"], raw["t"], raw["trace_voxels"] = np.ascontiguousarray(trace.T), (np.arange(n_steps) + 1) * dt, trace_voxels
    return dataset, raw
