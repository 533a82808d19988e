"""``run_fullwave_simulation`` -- full-wave FDTD field model (HIP kernel 5): reflection, refraction and transmission loss at the
interfaces of a heterogeneous medium, which the ray models (kernels 2a-2ph) leave out.

An opt-in model with the reference seam's leading arguments, so it can stand in for ``run_simulation`` where
``Protocol.calc_solution`` runs a replaced seam.  The model (DESIGN.md section 2 "full-wave model", kernel
section 5.14, fp64 oracle tests/fullwave_oracle.py): linear acoustics, first order in (p, v), on a staggered grid -- second order in
time, fourth order in space -- with narrow-band absorption exp(-2 alpha c dt) per step (alpha at the drive frequency), monopole
sources spread trilinearly over the 8 voxels around each element, and absorbing layers of ``pml_size`` voxels OUTSIDE ``params.coords``
(the medium is extended by edge replication, the results are cropped back).

With ``element_model="aperture"`` every element radiates (and, as a receiver, listens) over its finite rectangle: the rectangle is
sampled at ``upsampling_rate`` points per smallest voxel edge, each point spread trilinearly, the weights merged per (element, voxel) on
the device (fullwave_aperture_k; DESIGN.md section 2 "full-wave model: apertures", section 5.18).

``fullwave_time_axis``, ``layer_profile``, ``pad_volume`` / ``crop_volume``, ``source_table`` and ``aperture_geometry`` /
``check_apertures_inside`` are the host halves (pure functions); every refusal is raised before any device call."""
from __future__ import annotations

import logging

import numpy as np

from ..engine import Engine, get_engine, grid_from_coords
from ..util import dataset as ds
from ..util.units import getunitconversion
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


LAYER_MODELS = ("sponge", "pml")


def checked_layer_model(layer_model):
    """The model or ValueError: "sponge" (the multiplicative layers of ``layer_profile``) or "pml" (split perfectly matched layers,
    ``split_layer_tables``)."""
    if layer_model not in LAYER_MODELS:
        raise ValueError(f"full-wave simulation: layer_model must be one of {LAYER_MODELS}, got {layer_model!r}")
    return layer_model


def split_layer_tables(n_padded: int, spacing_m: float, pml_size: int, pml_alpha: float, c_ref: float, dt: float):
    """(r [n_padded], s [n_padded]) of one axis of the split layers (DESIGN.md section 2 "full-wave model: split layers"), fp64:
    r[i] = exp(-sigma(d_c(i)) dt / 2) with d_c = max(pml_size - i, i - (n - 1 - pml_size), 0) the depth of voxel i's centre, s[i] the same
    of the depth of its + face, d_f = max(pml_size - (i + 1/2), (i + 1/2) - (n - 1 - pml_size), 0); sigma(d) = pml_alpha (c_ref / h)
    (d / pml_size)^4.  Both are 1 in the interior, and everywhere with pml_size = 0."""
    n_padded, pml_size = int(n_padded), int(pml_size)
    if pml_size == 0:
        return np.ones(n_padded), np.ones(n_padded)
    i = np.arange(n_padded, dtype=np.float64)
    last = n_padded - 1 - pml_size
    k = float(pml_alpha) * (float(c_ref) / float(spacing_m))
    out = []
    for pos in (i, i + 0.5):
        x = np.maximum(np.maximum(pml_size - pos, pos - last), 0.0) / pml_size
        out.append(np.exp(-(k * x ** 4) * float(dt) / 2))
    return out[0], out[1]


def pad_volume(vol, pml_size: int):
    """[nx, ny, nz] -> the volume extended by ``pml_size`` voxels per side by edge replication."""
    return np.pad(np.asarray(vol), int(pml_size), mode="edge")


def crop_volume(vol, pml_size: int):
    """The inverse of ``pad_volume``: the caller's grid out of a padded volume."""
    q = int(pml_size)
    return np.ascontiguousarray(vol[q:vol.shape[0] - q, q:vol.shape[1] - q, q:vol.shape[2] - q]) if q else np.asarray(vol)


def trilinear_entries(pos_m, origin_m, spacing_m, n, snap: float = 1e-9, what: str = "element"):
    """The trilinear rule of the sources and of the receivers -> (ijk [S, 3] int64, weight [S], point [S]) on the caller's (unpadded) grid.

    Point e spreads over the 8 voxels around its position; weights of 0 are dropped, so a point exactly on a voxel gives one entry (a
    position within ``snap`` voxels of a voxel centre counts as on it).  A point with a weighted voxel outside the grid raises ValueError
    naming it as ``what``."""
    pos = np.atleast_2d(np.asarray(pos_m, dtype=np.float64))
    h = np.broadcast_to(np.asarray(spacing_m, dtype=np.float64), (3,))
    n = tuple(int(v) for v in n)
    ijk, wt, el = [], [], []
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
                        raise ValueError(f"full-wave simulation: {what} {e} at {tuple(pos[e])} m does not lie inside the grid "
                                         f"(its {'source ' if what == 'element' else ''}voxel {tuple(int(t) for t in v)} is outside {n})")
                    ijk.append(v); wt.append(w); el.append(e)
    return np.asarray(ijk, dtype=np.int64).reshape(-1, 3), np.asarray(wt, dtype=np.float64), np.asarray(el, dtype=np.int64)


def monopole_table(pos_m, A, delays, origin_m, spacing_m, n, sound_speed, freq, dt, snap: float = 1e-9, what: str = "element"):
    """Monopole source entries of points with free-field pressure A_e / r cos(2 pi freq (t - tau_e - r / c)) -> (ijk, amplitude, tau, point):
    amplitude = weight dt c(vox)^2 4 pi A_e / (2 pi freq h_x h_y h_z), in the order of ``trilinear_entries``."""
    h = np.broadcast_to(np.asarray(spacing_m, dtype=np.float64), (3,))
    cs = np.asarray(sound_speed, dtype=np.float64)
    A, tau = np.asarray(A, dtype=np.float64), np.asarray(delays, dtype=np.float64)
    scale = float(dt) * 4.0 * np.pi / (2.0 * np.pi * float(freq) * float(np.prod(h)))
    ijk, wt, el = trilinear_entries(pos_m, origin_m, h, n, snap, what)
    c_v = np.full(el.shape, float(cs)) if cs.ndim == 0 else cs[tuple(ijk.T)].astype(np.float64)
    amp = np.asarray([w * scale * c * c * A[e] for w, c, e in zip(wt, c_v, el)], dtype=np.float64)
    return ijk, amp, tau[el].astype(np.float64), el


def source_table(pos_m, area, apod, delays, origin_m, spacing_m, n, sound_speed, c_ref, freq, p0, dt, snap: float = 1e-9):
    """Monopole source entries on the caller's (unpadded) grid -> (ijk [S, 3] int64, amplitude [S], tau [S], element [S]).

    Element e contributes to the 8 voxels around its position with trilinear weights; weights of 0 are dropped, so an element
    exactly on a voxel gives one entry (a position within ``snap`` voxels of a voxel centre counts as on it).  amplitude =
    weight dt c(vox)^2 4 pi A_e / (2 pi freq h_x h_y h_z) with A_e = apod_e p0 area_e freq / c_ref: the monopole whose free-field
    pressure is A_e / r cos(2 pi freq (t - tau_e - r / c)).  An element with a weighted voxel outside the grid raises ValueError."""
    A = np.asarray(apod, dtype=np.float64) * np.asarray(area, dtype=np.float64) * float(p0) * float(freq) / float(c_ref)
    return monopole_table(pos_m, A, delays, origin_m, spacing_m, n, sound_speed, freq, dt, snap)


def receiver_table(points_m, origin_m, spacing_m, n, snap: float = 1e-9):
    """CSR receiver table on the caller's (unpadded) grid -> (row [R + 1] int32, ijk [S, 3] int64, weight [S]): receiver r reads
    sum_q weight[q] p(ijk[q]) over q in [row[r], row[r + 1]), the trilinear rule of ``source_table``."""
    pts = np.asarray(points_m, dtype=np.float64)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError(f"receivers must have shape (P, 3), got {pts.shape}")
    if not np.all(np.isfinite(pts)):
        raise ValueError("full-wave simulation: receiver positions must be finite")
    if pts.shape[0] == 0:
        return np.zeros(1, dtype=np.int32), np.zeros((0, 3), dtype=np.int64), np.zeros(0)
    ijk, wt, el = trilinear_entries(pts, origin_m, spacing_m, n, snap, "receiver")
    row = np.concatenate([[0], np.cumsum(np.bincount(el, minlength=pts.shape[0]))]).astype(np.int32)
    return row, ijk, wt


# ---- finite rectangular element apertures (DESIGN.md section 2 "full-wave model: apertures", kernels section 5.18) ------------------
ELEMENT_MODELS = ("point", "aperture")
MAX_APERTURE_POINTS = 65536


def checked_element_model(element_model, upsampling_rate=5):
    """(model, rate) or ValueError: the model is "point" (one trilinear monopole per element) or "aperture" (the element's rectangle
    sampled at ``upsampling_rate`` points per smallest voxel edge); the rate is an integer >= 1."""
    if element_model not in ELEMENT_MODELS:
        raise ValueError(f"full-wave simulation: element_model must be one of {ELEMENT_MODELS}, got {element_model!r}")
    r = upsampling_rate
    if isinstance(r, bool) or not isinstance(r, (int, np.integer)) or r < 1:
        raise ValueError(f"full-wave simulation: upsampling_rate must be an integer >= 1, got {upsampling_rate!r}")
    return element_model, int(r)


def aperture_counts(size_m, spacing_m, upsampling_rate: int = 5):
    """(n_w [E], n_l [E]) int32: n = max(1, ceil(rate size / h_min - 1e-9)) quadrature points along the width and the length.  More than
    65536 points for one element raises ValueError."""
    _, rate = checked_element_model("aperture", upsampling_rate)
    size = np.asarray(size_m, dtype=np.float64).reshape(-1, 2)
    if not (np.all(np.isfinite(size)) and np.all(size >= 0)):
        raise ValueError("full-wave simulation: element sizes must be finite and >= 0")
    h_min = float(np.min(np.broadcast_to(np.asarray(spacing_m, dtype=np.float64), (3,))))
    cnt = np.maximum(1.0, np.ceil(rate * size / h_min - 1e-9))
    pts = cnt[:, 0] * cnt[:, 1]
    if np.any(pts > MAX_APERTURE_POINTS):
        e = int(np.argmax(pts > MAX_APERTURE_POINTS))
        raise ValueError(f"full-wave simulation: element {e} of {size[e, 0]:g} x {size[e, 1]:g} m takes {int(pts[e])} quadrature points at "
                         f"upsampling_rate {rate} (at most {MAX_APERTURE_POINTS})")
    return cnt[:, 0].astype(np.int32), cnt[:, 1].astype(np.int32)


def aperture_geometry(arr, spacing_m, upsampling_rate: int = 5, transform=None):
    """The rectangles of ``arr``'s elements -> dict(centre [E, 3] m, u [E, 3], v [E, 3], size [E, 2] m, n_w [E], n_l [E]): u = R[:, 0]
    (width) and v = R[:, 1] (length) of R = rotation_from_angles(az, el, roll), centre and axes after ``transform`` (4 x 4, metres)."""
    from ..xdc.element import rotation_from_angles
    els = arr.elements
    centre = np.asarray(arr.element_table()[0], dtype=np.float64).reshape(-1, 3)
    ori = np.array([el.orientation for el in els], dtype=np.float64).reshape(-1, 3)
    R = rotation_from_angles(ori[:, 0], ori[:, 1], ori[:, 2]).reshape(-1, 3, 3)
    u, v = np.ascontiguousarray(R[:, :, 0]), np.ascontiguousarray(R[:, :, 1])
    size = np.array([[s * getunitconversion(el.units, "m") for s in el.size] for el in els], dtype=np.float64).reshape(-1, 2)
    if transform is not None:
        M = np.asarray(transform, dtype=np.float64)
        if M.shape != (4, 4):
            raise ValueError(f"transform must be a 4 x 4 matrix, got {M.shape}")
        centre, u, v = centre @ M[:3, :3].T + M[:3, 3], u @ M[:3, :3].T, v @ M[:3, :3].T
    n_w, n_l = aperture_counts(size, spacing_m, upsampling_rate)
    return {"centre": centre, "u": u, "v": v, "size": size, "n_w": n_w, "n_l": n_l}


def aperture_points(geom, e: int):
    """x_ab [n_w n_l, 3] m of element ``e``: c + ((a + 1/2) / n_w - 1/2) w u + ((b + 1/2) / n_l - 1/2) l v, a outer, b inner."""
    nw, nl = int(geom["n_w"][e]), int(geom["n_l"][e])
    sa = np.repeat((np.arange(nw) + 0.5) / nw - 0.5, nl)[:, None]
    sb = np.tile((np.arange(nl) + 0.5) / nl - 0.5, nw)[:, None]
    return (geom["centre"][e] + (sa * geom["size"][e, 0]) * geom["u"][e]) + (sb * geom["size"][e, 1]) * geom["v"][e]


def check_apertures_inside(geom, origin_m, spacing_m, n, snap: float = 1e-9, what: str = "element"):
    """ValueError naming the first element with a weighted voxel outside the grid ``n`` -- the refusal of ``trilinear_entries`` for every
    quadrature point, decided on the host from the extreme points (the others lie between them on every axis)."""
    h = np.broadcast_to(np.asarray(spacing_m, dtype=np.float64), (3,))
    o = np.asarray(origin_m, dtype=np.float64)
    for name in ("centre", "u", "v", "size"):
        if not np.all(np.isfinite(geom[name])):
            raise ValueError(f"full-wave simulation: {what} {name} must be finite")
    nw, nl = geom["n_w"].astype(np.float64), geom["n_l"].astype(np.float64)
    lo, hi = np.full(geom["centre"].shape, np.inf), np.full(geom["centre"].shape, -np.inf)
    for ea in (0, 1):
        for eb in (0, 1):
            sa = ((nw - 1 if ea else 0 * nw) + 0.5) / nw - 0.5
            sb = ((nl - 1 if eb else 0 * nl) + 0.5) / nl - 0.5
            x = (geom["centre"] + (sa * geom["size"][:, 0])[:, None] * geom["u"]) + (sb * geom["size"][:, 1])[:, None] * geom["v"]
            q = (x - o) / h
            near = np.rint(q)
            q = np.where(np.abs(q - near) <= snap, near, q)
            lo, hi = np.minimum(lo, q), np.maximum(hi, q)
    bad = np.any((lo < 0) | (np.ceil(hi) > np.asarray(n, dtype=np.float64) - 1), axis=1)
    if np.any(bad):
        e = int(np.argmax(bad))
        raise ValueError(f"full-wave simulation: {what} {e} at {tuple(geom['centre'][e])} m does not lie inside the grid (its aperture spans "
                         f"voxels {tuple(np.round(lo[e], 3))} .. {tuple(np.round(hi[e], 3))} of {tuple(int(v) for v in n)})")


def aperture_table(geom, origin_m, spacing_m, n):
    """The aperture weights of ``geom`` (``aperture_geometry``) on the grid (origin, spacing, n) -> per-element CSR (row [E + 1] int32,
    ijk [S, 3] int64, weight [S] float64): W_e(m) = 1 / (n_w n_l) sum_a sum_b prod_axis max(0, 1 - |q_ab - m|), the trilinear spread of
    the element's quadrature points merged per voxel (sum_m W_e(m) = 1; n_w = n_l = 1 is ``trilinear_entries``' rule).  The host side of
    olx_fullwave_apertures (fullwave_aperture_k evaluates the weights): it plans a uniform medium on this grid, so a full-wave plan that
    was resident is replaced.  Every refusal is raised before any device call."""
    n = tuple(int(v) for v in n)
    h = np.broadcast_to(np.asarray(spacing_m, dtype=np.float64), (3,))
    check_apertures_inside(geom, origin_m, h, n)
    ctx = get_engine().ctx
    ctx.fullwave_plan(h, n, 1500.0, 1000.0, 0.0, 1500.0, 0, 0.0, 0.5 * stability_bound(h, 1500.0))
    row, vox, wt = ctx.fullwave_apertures(geom["centre"] - np.asarray(origin_m, dtype=np.float64), geom["u"], geom["v"], geom["size"], geom["n_w"], geom["n_l"])
    return row, np.stack(np.unravel_index(vox, n), axis=1).astype(np.int64).reshape(-1, 3), wt


def _padded_geometry(geom, origin_m, spacing_m, pml_size):
    """``geom`` as Engine.fullwave takes it: centres in the frame of the padded grid (its voxel 0 at 0)."""
    h = np.broadcast_to(np.asarray(spacing_m, dtype=np.float64), (3,))
    return (geom["centre"] - (np.asarray(origin_m, dtype=np.float64) - int(pml_size) * h), geom["u"], geom["v"], geom["size"], geom["n_w"], geom["n_l"])


def _layer_kw(layer_model):
    """The engine's keyword for a layer model that is not the default (the default call stays the one it was)."""
    return {} if layer_model == "sponge" else {"layer_model": layer_model}


DRIVE_MODELS = ("impulse_response",)      # what drives the elements besides the bare burst, opt-in (DESIGN.md section 2 "full-wave model: drives")


def checked_drive_model(drive_model):
    """The model or ValueError: None (the bare burst; the transducer's impulse responses are ignored) or "impulse_response"."""
    if drive_model is not None and drive_model not in DRIVE_MODELS:
        raise ValueError(f'full-wave simulation: drive_model must be None or one of {DRIVE_MODELS}, got {drive_model!r}')
    return drive_model


def response_of(arr, dt):
    """The drive taps of ``arr`` on the ``dt`` grid as the full-wave model takes them -> (class_of_element int32 [E], [taps_c], M [E] taps of
    each element's class), or None for a transducer without any response.  sim/field.py ``drive_taps`` with one class per element allowed."""
    from .field import drive_taps
    cls, taps = drive_taps(arr, dt, max_classes=max(1, arr.numelements()), what="full-wave simulation")
    if not taps:
        return None
    return cls, taps, np.asarray([len(taps[c]) for c in cls], dtype=np.int64)


def checked_source_waveforms(source_waveforms, n_el, dt, delays, drive_model):
    """``source_waveforms`` as a float64 [n_el, n_t] array, or ValueError: it needs an explicit dt > 0 and no delays, and excludes
    ``drive_model``."""
    if drive_model is not None:
        raise ValueError("full-wave simulation: source_waveforms and drive_model exclude each other (a sampled waveform carries its own response)")
    if delays is not None:
        raise ValueError("full-wave simulation: source_waveforms take no delays (delay the waveforms themselves)")
    if not (np.isfinite(dt) and dt > 0):
        raise ValueError(f"full-wave simulation: source_waveforms are samples on the step grid and need an explicit dt > 0, got {dt}")
    W = np.asarray(source_waveforms, dtype=np.float64)
    if W.ndim != 2 or W.shape[0] != n_el or W.shape[1] < 1:
        raise ValueError(f"source_waveforms must have shape ({n_el}, n_t) with n_t >= 1, got {W.shape}")
    if not np.all(np.isfinite(W)):
        raise ValueError("full-wave simulation: source_waveforms must be finite")
    return W


def _broadcast(value, ref, shape):
    return np.full(shape, ref, dtype=np.float64) if value is None else np.asarray(value, dtype=np.float64)


def _medium_of(params, freq, ref_values_only):
    """(c_ref, rho_ref, sound speed, density, absorption [Np/m]), each of the last three a float or a volume of the caller's grid."""
    c_ref, rho_ref, medium, absorption = _medium(params, freq, ref_values_only)
    if medium is None:      # homogeneous: the uniform instantiation streams no coefficient volume
        return c_ref, rho_ref, c_ref, rho_ref, float(absorption)
    cs = c_ref if medium["sound_speed"] is None else np.asarray(medium["sound_speed"], dtype=np.float64)
    rho = rho_ref if medium["density"] is None else np.asarray(medium["density"], dtype=np.float64)
    alpha = 0.0 if medium["attenuation"] is None else np.asarray(medium["attenuation"], dtype=np.float64) * _np_per_m(1.0, freq)
    return c_ref, rho_ref, cs, rho, alpha


def _impedance(params, ref_values_only, c_ref, rho_ref, cs, rho):
    """The impedance of the intensity: the volumes' own rho c (with ref_values_only too, as run_simulation forms it)."""
    if ref_values_only:
        uniform = all(getattr(params[k], "uniform_value", None) is not None for k in ("density", "sound_speed"))
        return rho_ref * c_ref if uniform else np.asarray(params["density"].data, dtype=np.float64) * np.asarray(params["sound_speed"].data, dtype=np.float64)
    return np.asarray(rho, dtype=np.float64) * np.asarray(cs, dtype=np.float64)


def run_fullwave_simulation(arr, params, delays=None, apod=None, freq: float = 1e6, cycles: float = 20, amplitude: float = 1,
                            dt: float = 0, t_end: float = 0, cfl: float = 0.3, bli_tolerance: float = 0.05, upsampling_rate: int = 5,
                            gpu: bool = True, ref_values_only: bool = False, *, pml_size: int = 16, pml_alpha: float = 2.0,
                            ramp_cycles: float = 0.0, pulse_intensity_integral: bool = False, record_points=None, element_model: str = "point",
                            layer_model: str = "sponge", drive_model=None, source_waveforms=None):
    """Full-wave simulation of one steering -> (Dataset{p_max [Pa], p_min [Pa], intensity [W/cm^2]} on ``params.coords``, raw).

    The leading arguments are ``run_simulation``'s; ``gpu`` is accepted and ignored (there is no CPU path).  ``element_model`` "point"
    (the default) makes every element one trilinear monopole and ignores ``upsampling_rate``; "aperture" radiates from the element's
    rectangle, sampled at ``upsampling_rate`` points per smallest voxel edge (``aperture_table``).  ``bli_tolerance`` is ignored by both:
    the spread is trilinear, not band-limited.  ``raw`` names the model and, for "aperture", its number of (element, voxel) entries.
    ``delays`` are used as given (no truncation to whole steps).  intensity = 1e-4 p_min^2 / (2 rho c) and, with
    ``pulse_intensity_integral``, PII = 1e-4 dt sum p^2 / (rho c) [J/cm^2], both with the voxel's own rho c.  ``record_points`` [P, 3] in
    the coordinates' units adds "p_trace" [P, n_steps] (p after each step), "t" and "trace_voxels" to ``raw``.  ``layer_model`` "sponge"
    (the default) damps every field of a layer voxel each step; "pml" runs split perfectly matched layers (``split_layer_tables``), which
    leave a wave travelling along a layer alone, so a grid cropped narrowly around the beam keeps its on-axis amplitude;
    ``raw["layer_model"]`` reports it.

    ``drive_model`` None (the default) drives every element with the bare tone burst: the ``impulse_response`` of the transducer and of its
    elements is ignored.  "impulse_response" opts in to them: element e's drive is sum_m g_e[m] burst((n - m) dt) with the drive taps
    g_e = H_arr * H_el,e of sim/field.py ``drive_taps`` on the run's dt grid (at most 256 taps; every element may have its own), formed on the
    device (fullwave_drive_fir_k; DESIGN.md section 2 "full-wave model: drives").  Both element models then go through the element-factored source form;
    a transducer without any response runs the default path.  With ``t_end = 0`` the run grows by the longest response.
    ``source_waveforms`` [n_el, n_t] drives element e with the samples A_e W[e, n] at step n, in units of the bare burst -- sin(2 pi freq
    (n - 1/2) dt) reproduces a CW drive -- padded with zeros to n_steps = max(n_t, ceil(t_end / dt)); it needs an explicit ``dt``, takes no
    ``delays``, ignores ``cycles`` and ``ramp_cycles`` and excludes ``drive_model``.  ``raw["drive_model"]`` ("impulse_response",
    "source_waveforms" or None) and ``raw["drive_taps"]`` (the largest number of taps, None without the opt-in) report the drive."""
    element_model, upsampling_rate = checked_element_model(element_model, upsampling_rate if element_model == "aperture" else 1)
    layer_model = checked_layer_model(layer_model)
    drive_model = checked_drive_model(drive_model)
    n_el = arr.numelements()
    W = None if source_waveforms is None else checked_source_waveforms(source_waveforms, n_el, float(dt), delays, drive_model)
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
    c_ref, rho_ref, cs, rho, alpha = _medium_of(params, freq, ref_values_only)
    response = table = None
    if W is not None:
        # the samples are the run: n_steps = max(n_t, ceil(t_end / dt)); the burst's length means nothing here (cycles = 1 passes the checks)
        cycles, ramp_cycles = 1.0, 0.0
        dt, n_steps, dt_max, ppw = fullwave_time_axis(spacing, n, cs, freq, cycles, 0.0, dt, t_end if float(t_end) > 0 else W.shape[1] * float(dt), cfl)
        n_steps = max(W.shape[1], n_steps if float(t_end) > 0 else 0)
        if n_steps >= 2 ** 31:
            raise ValueError(f"full-wave simulation: {n_steps} steps is too many")
    elif drive_model is not None:
        # dt does not depend on the delays: form it first, resample the responses to it, then let the run end M_e - 1 steps later for element e
        dt = fullwave_time_axis(spacing, n, cs, freq, cycles, delays, dt, t_end, cfl)[0]
        response = response_of(arr, dt)
        lead = 0.0 if response is None else (response[2] - 1) * dt
        dt, n_steps, dt_max, ppw = fullwave_time_axis(spacing, n, cs, freq, cycles, delays + lead, dt, t_end, cfl)
    else:
        dt, n_steps, dt_max, ppw = fullwave_time_axis(spacing, n, cs, freq, cycles, delays, dt, t_end, cfl)
    factored = response is not None or W is not None      # the element-factored source form: its drive table is where both drives go
    pos, _, area, _ = Engine._table_of(arr)
    p0 = float(amplitude) * (1.0 if arr.sensitivity is None else float(arr.sensitivity))
    if element_model == "aperture" or factored:
        A = apod * np.asarray(area, dtype=np.float64) * p0 * float(freq) / float(c_ref)
    if element_model == "aperture":
        geom = aperture_geometry(arr, spacing, upsampling_rate)
        check_apertures_inside(geom, origin, spacing, n)
    elif factored:
        ijk, amp, _, el = monopole_table(pos, np.ones(n_el), delays, origin, spacing, n, cs, freq, dt)
    else:
        ijk, amp, tau, _ = source_table(pos, area, apod, delays, origin, spacing, n, cs, c_ref, freq, p0, dt)
    if W is not None:
        table = np.zeros((n_steps, n_el))
        table[:W.shape[1]] = (A[:, None] * W).T
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
    if element_model == "aperture":
        sources = {"geometry": _padded_geometry(geom, origin, spacing, pml_size), "A": A, "tau": delays}
    elif factored:
        sources = {"voxels": lin(ijk), "elements": el, "amplitude": amp, "A": A, "tau": delays}
    else:
        sources = (lin(ijk), amp, tau)
    if response is not None:
        sources["response"] = response[:2]
    if table is not None:
        sources["table"] = table
    pmax, pmin, psq, trace = eng.fullwave(spacing, npad, vols, c_ref, pml_size, pml_alpha, dt, n_steps, sources, freq, cycles,
                                          ramp_cycles, psq=bool(pulse_intensity_integral), points=None if tr_ijk is None else lin(tr_ijk),
                                          **_layer_kw(layer_model))
    logging.info("Simulation Complete")
    pmax, pmin = crop_volume(pmax, pml_size), crop_volume(pmin, pml_size)
    Z = _impedance(params, ref_values_only, c_ref, rho_ref, cs, rho)
    inten = (1e-4 * pmin.astype(np.float64) ** 2 / (2.0 * Z)).astype(np.float32)
    dims = list(coords.dims) if hasattr(coords, "dims") else list(coords.keys())
    out = {"p_max": ds.make_dataarray(pmax, coords=coords, dims=dims, name="p_max", attrs=_ATTRS["p_max"]),
           "p_min": ds.make_dataarray(pmin.copy(), coords=coords, dims=dims, name="p_min", attrs=_ATTRS["p_min"]),
           "intensity": ds.make_dataarray(inten, coords=coords, dims=dims, name="I", attrs=_ATTRS["intensity"])}
    dataset = ds.make_dataset(out)
    raw = {"p_max": pmax, "p_min": -pmin, "dt": dt, "n_steps": n_steps, "dt_max": dt_max, "points_per_wavelength": ppw,
           "backend": "openlifu_amd/hip-gfx950", "element_model": element_model, "layer_model": layer_model,
           "aperture_entries": eng.fullwave_aperture_entries if element_model == "aperture" else None,
           "drive_model": "source_waveforms" if W is not None else drive_model,
           "drive_taps": None if drive_model is None else 1 if response is None else int(response[2].max())}
    if pulse_intensity_integral:
        pii = (1e-4 * dt * crop_volume(psq, pml_size).astype(np.float64) / Z).astype(np.float32)
        dataset["pulse_intensity_integral"] = ds.make_dataarray(pii, coords=coords, dims=dims, name="pulse_intensity_integral",
                                                                attrs=_ATTRS["pulse_intensity_integral"])
        raw["pulse_intensity_integral"] = pii
    if trace_voxels is not None:
        raw["p_trace"], raw["t"], raw["trace_voxels"] = np.ascontiguousarray(trace.T), (np.arange(n_steps) + 1) * dt, trace_voxels
    return dataset, raw


# ---- steady state at the drive frequency: single-frequency lock-in over the last cycles of a driven run ----
PHASE_ATTRS = {"units": "cycles", "long_name": "Phase lag behind sin(2 pi f0 t)"}


def lockin_window(n_steps: int, dt: float, freq: float, lockin_cycles: float):
    """(w0, Nw): the last Nw = rint(lockin_cycles / (freq dt)) steps of a run of ``n_steps``.  ValueError when Nw < 1 or the window does
    not fit the run."""
    x = float(lockin_cycles) / (float(freq) * float(dt))
    if not (np.isfinite(x) and x > 0):
        raise ValueError(f"full-wave steady state: lockin_cycles must be finite and > 0, got {lockin_cycles}")
    nw = int(np.rint(x))
    if nw < 1:
        raise ValueError(f"full-wave steady state: a window of {lockin_cycles} cycles holds no step of dt = {dt:g} s")
    if nw > int(n_steps):
        raise ValueError(f"full-wave steady state: a window of {nw} steps ({lockin_cycles} cycles) does not fit the run of {n_steps} steps")
    return int(n_steps) - nw, nw


def lockin_angles(freq: float, dt: float, w0: int, nw: int):
    """theta_n = 2 pi frac(freq t_n), t_n = (n + 1) dt, for the steps n of the window."""
    ph = float(freq) * ((np.arange(int(w0), int(w0) + int(nw), dtype=np.float64) + 1.0) * float(dt))
    return 2.0 * np.pi * (ph - np.floor(ph))


def lockin_amplitude_phase(C, S, nw: int):
    """Sums over a window of ``nw`` steps -> (amplitude A = 2 / nw hypot(C, S), lag psi = atan2(-C, S) / 2 pi [cycles] in (-1/2, 1/2]),
    fp64: psi is the lag of p behind sin(2 pi f0 t), so a wave with travel time T has psi = f0 T (mod 1)."""
    C, S = np.asarray(C, dtype=np.float64), np.asarray(S, dtype=np.float64)
    psi = np.arctan2(-C, S) / (2.0 * np.pi)
    return 2.0 / int(nw) * np.hypot(C, S), np.where(psi <= -0.5, 0.5, psi)


def steady_state_run(params, pos_m, A, tau, freq, dt=0.0, t_end=0.0, cfl=0.3, ref_values_only=False, lockin_cycles=4, settle_cycles=3,
                     ramp_cycles=2.0, pml_size=16, pml_alpha=2.0, receivers_m=None, volume=True, what="element", apertures=None,
                     receiver_apertures=None, *, layer_model="sponge", drive_model=None, arr=None):
    """One driven run of monopoles (``pos_m`` [E, 3] m, free-field amplitude ``A`` [Pa m], delay ``tau`` [s]) with the lock-in over its
    last ``lockin_cycles`` cycles -> dict(C, S (cropped volumes or None), rec_C, rec_S (float64 [R] or None), dt, n_steps, window,
    points_per_wavelength, cycles, t_end, medium = (c_ref, rho_ref, cs, rho), aperture_entries).  ``apertures`` (``aperture_geometry``)
    makes the sources the elements' rectangles, ``pos_m`` being ignored; ``receiver_apertures`` makes the receivers the aperture averages
    sum_m W_e(m) p(m) of those rectangles in place of ``receivers_m``.  ``layer_model`` is ``run_fullwave_simulation``'s.
    ``drive_model="impulse_response"`` drives the monopoles through the impulse responses of the transducer ``arr`` (``response_of``; one
    monopole per element of ``arr``): the default ``t_end`` grows by (M_max - 1) dt and the dict gains "drive_taps" = M_max.  Every refusal
    is raised before any device call."""
    layer_model = checked_layer_model(layer_model)
    drive_model = checked_drive_model(drive_model)
    if drive_model is not None and arr is None:
        raise ValueError("full-wave steady state: drive_model needs the transducer whose impulse responses drive the elements (arr)")
    pml_size = int(pml_size)
    if pml_size < 0 or not (np.isfinite(pml_alpha) and pml_alpha >= 0):
        raise ValueError(f"full-wave simulation: pml_size must be >= 0 and pml_alpha finite and >= 0, got {pml_size}, {pml_alpha}")
    for name, v in (("lockin_cycles", lockin_cycles), ("settle_cycles", settle_cycles), ("ramp_cycles", ramp_cycles)):
        if not (np.isfinite(v) and v >= 0):
            raise ValueError(f"full-wave steady state: {name} must be finite and >= 0, got {v}")
    if not lockin_cycles > 0:
        raise ValueError(f"full-wave steady state: lockin_cycles must be > 0, got {lockin_cycles}")
    coords = params.coords
    origin, spacing, n = grid_from_coords(coords)
    n = tuple(int(v) for v in n)
    c_ref, rho_ref, cs, rho, alpha = _medium_of(params, freq, ref_values_only)
    tau = np.asarray(tau, dtype=np.float64)
    total = float(ramp_cycles) + float(settle_cycles) + float(lockin_cycles)
    dt, n_steps, dt_max, ppw = fullwave_time_axis(spacing, n, cs, freq, total, tau, dt, t_end, cfl)
    response, lead = None, 0.0
    if drive_model is not None:
        response = response_of(arr, dt)
        if response is not None:
            if response[0].shape != tau.shape:
                raise ValueError(f"full-wave steady state: the transducer has {response[0].size} elements, the run {tau.size} monopoles")
            lead = float(response[2].max() - 1) * dt
            if lead > 0:      # the longest response reaches that far behind the burst: the default run waits for it
                dt, n_steps, dt_max, ppw = fullwave_time_axis(spacing, n, cs, freq, total, tau + lead, dt, t_end, cfl)
    t_end = float(t_end)
    if t_end == 0:      # (the default fullwave_time_axis has just taken: |n h| / c_min + max tau + total / freq, plus the longest response)
        h = np.broadcast_to(np.asarray(spacing, dtype=np.float64), (3,))
        t_end = (float(np.sqrt(np.sum((np.asarray(n, dtype=np.float64) * h) ** 2))) / float(np.min(cs)) + (float(tau.max()) if tau.size else 0.0)
                 + total / float(freq))
        if lead > 0:
            t_end += lead
    cycles = float(np.ceil(float(freq) * t_end) + 1.0)      # the drive lasts through the end of the run
    w0, nw = lockin_window(n_steps, dt, freq, lockin_cycles)
    if apertures is not None:
        check_apertures_inside(apertures, origin, spacing, n, what=what)
        sources = {"geometry": _padded_geometry(apertures, origin, spacing, pml_size), "A": np.asarray(A, dtype=np.float64), "tau": tau}
    elif response is not None:      # the element-factored form carries the drive table the response goes into
        ijk, amp, _, el = monopole_table(pos_m, np.ones(tau.shape), tau, origin, spacing, n, cs, freq, dt, what=what)
    else:
        ijk, amp, tt, _ = monopole_table(pos_m, A, tau, origin, spacing, n, cs, freq, dt, what=what)
    row = r_ijk = r_w = None
    if receiver_apertures is not None:
        check_apertures_inside(receiver_apertures, origin, spacing, n, what="receiver")
    elif receivers_m is not None:
        row, r_ijk, r_w = receiver_table(receivers_m, origin, spacing, n)
    if not volume and row is None and receiver_apertures is None:
        raise ValueError("full-wave steady state: neither the volume nor a receiver to record")
    npad = tuple(v + 2 * pml_size for v in n)

    def lin(v):
        v = v + pml_size
        return (v[:, 0] * npad[1] + v[:, 1]) * npad[2] + v[:, 2]

    vols = [v if np.ndim(v) == 0 else pad_volume(v, pml_size) for v in (cs, rho, alpha)]
    logging.info("Running full-wave steady-state simulation")
    eng = get_engine()
    if apertures is None and response is not None:
        sources = {"voxels": lin(ijk), "elements": el, "amplitude": amp, "A": np.asarray(A, dtype=np.float64), "tau": tau}
    elif apertures is None:
        sources = (lin(ijk), amp, tt)
    if response is not None:
        sources["response"] = response[:2]
    if receiver_apertures is not None:
        receivers = {"geometry": _padded_geometry(receiver_apertures, origin, spacing, pml_size)}
    else:
        receivers = None if row is None else (row, lin(r_ijk), r_w)
    vc, vs, rc, rs = eng.fullwave_steady(spacing, npad, vols, c_ref, pml_size, pml_alpha, dt, n_steps, sources, freq, cycles, ramp_cycles,
                                         window=(w0, nw), volume=bool(volume), receivers=receivers, **_layer_kw(layer_model))
    logging.info("Simulation Complete")
    if receivers is not None and rc is None:      # an empty receiver table
        rc = rs = np.zeros(0)
    return {"C": None if vc is None else crop_volume(vc, pml_size), "S": None if vs is None else crop_volume(vs, pml_size), "rec_C": rc, "rec_S": rs,
            "dt": dt, "n_steps": n_steps, "dt_max": dt_max, "window": (w0, nw), "points_per_wavelength": ppw, "cycles": cycles, "t_end": t_end,
            "medium": (c_ref, rho_ref, cs, rho), "aperture_entries": eng.fullwave_aperture_entries,
            "drive_taps": None if drive_model is None else 1 if response is None else int(response[2].max())}


def run_fullwave_steady_state(arr, params, delays=None, apod=None, freq: float = 1e6, amplitude: float = 1, dt: float = 0, t_end: float = 0,
                              cfl: float = 0.3, ref_values_only: bool = False, *, lockin_cycles: float = 4, settle_cycles: float = 3,
                              ramp_cycles: float = 2.0, pml_size: int = 16, pml_alpha: float = 2.0, receivers=None, element_model: str = "point",
                              upsampling_rate: int = 5, layer_model: str = "sponge", drive_model=None):
    """Steady state of one steering at the drive frequency -> (Dataset{p_max = p_min = A [Pa], intensity [W/cm^2], phase [cycles]} on
    ``params.coords``, raw): the full-wave model driven through the end of the run, locked in at ``freq`` over its last ``lockin_cycles``
    cycles (DESIGN.md section 2 "full-wave model", kernel section 5.15).

    The drive ramps up over ``ramp_cycles`` and lasts ceil(freq t_end) + 1 cycles; t_end = 0 gives |n h| / c_min + max(delays) +
    (ramp_cycles + settle_cycles + lockin_cycles) / freq.  The window is the last Nw = rint(lockin_cycles / (freq dt)) steps.  With the
    sums C = sum p cos(theta_n), S = sum p sin(theta_n) over it, A = 2 / Nw hypot(C, S) and phase = atan2(-C, S) / 2 pi in (-1/2, 1/2],
    the lag of p behind sin(2 pi freq t); Nw freq dt is not a whole number, so both carry a leakage of the order 1 / (2 Nw) that nothing
    corrects.  intensity = 1e-4 A^2 / (2 rho c) with the impedance rules of ``run_fullwave_simulation``.  ``receivers`` [P, 3] in the
    coordinates' units adds "receiver_amplitude", "receiver_phase" and "receiver_sums" (C_r + i S_r, trilinear weights) to ``raw``.
    ``element_model`` / ``upsampling_rate`` / ``layer_model`` / ``drive_model`` are ``run_fullwave_simulation``'s: with
    ``drive_model="impulse_response"`` the steady state carries the responses' gain and lag at ``freq``, and the default ``t_end`` grows by
    (M_max - 1) dt; ``raw["drive_model"]`` and ``raw["drive_taps"]`` report the drive."""
    element_model, upsampling_rate = checked_element_model(element_model, upsampling_rate if element_model == "aperture" else 1)
    layer_model = checked_layer_model(layer_model)
    drive_model = checked_drive_model(drive_model)
    n_el = arr.numelements()
    delays = np.zeros(n_el) if delays is None else np.asarray(delays, dtype=np.float64)
    apod = np.ones(n_el) if apod is None else np.asarray(apod, dtype=np.float64)
    if delays.shape != (n_el,) or apod.shape != (n_el,):
        raise ValueError(f"delays and apod must have shape ({n_el},), got {delays.shape} and {apod.shape}")
    if not (np.all(np.isfinite(delays)) and np.all(np.isfinite(apod))):
        raise ValueError("full-wave simulation: delays and apod must be finite")
    coords = params.coords
    rec_m = None
    if receivers is not None:
        dims = list(coords.dims) if hasattr(coords, "dims") else list(coords.keys())
        rec = np.asarray(receivers, dtype=np.float64)
        if rec.ndim != 2 or rec.shape[1] != 3:
            raise ValueError(f"receivers must have shape (P, 3), got {rec.shape}")
        rec_m = rec * getunitconversion(coords[dims[0]].attrs["units"], "m")
    pos, _, area, _ = Engine._table_of(arr)
    p0 = float(amplitude) * (1.0 if arr.sensitivity is None else float(arr.sensitivity))
    c_ref = float(params["sound_speed"].attrs["ref_value"])
    A0 = apod * np.asarray(area, dtype=np.float64) * p0 * float(freq) / c_ref
    geom = aperture_geometry(arr, grid_from_coords(coords)[1], upsampling_rate) if element_model == "aperture" else None
    run = steady_state_run(params, pos, A0, delays, freq, dt, t_end, cfl, ref_values_only, lockin_cycles, settle_cycles, ramp_cycles, pml_size,
                           pml_alpha, receivers_m=rec_m, volume=True, apertures=geom, **_layer_kw(layer_model),
                           **({} if drive_model is None else {"drive_model": drive_model, "arr": arr}))
    w0, nw = run["window"]
    A, psi = lockin_amplitude_phase(run["C"], run["S"], nw)
    c_ref, rho_ref, cs, rho = run["medium"]
    Z = _impedance(params, ref_values_only, c_ref, rho_ref, cs, rho)
    inten = (1e-4 * A ** 2 / (2.0 * Z)).astype(np.float32)
    A32, psi32 = A.astype(np.float32), psi.astype(np.float32)
    dims = list(coords.dims) if hasattr(coords, "dims") else list(coords.keys())
    out = {"p_max": ds.make_dataarray(A32, coords=coords, dims=dims, name="p_max", attrs=_ATTRS["p_max"]),
           "p_min": ds.make_dataarray(A32.copy(), coords=coords, dims=dims, name="p_min", attrs=_ATTRS["p_min"]),
           "intensity": ds.make_dataarray(inten, coords=coords, dims=dims, name="I", attrs=_ATTRS["intensity"]),
           "phase": ds.make_dataarray(psi32, coords=coords, dims=dims, name="phase", attrs=PHASE_ATTRS)}
    raw = {"dt": run["dt"], "n_steps": run["n_steps"], "dt_max": run["dt_max"], "window": (w0, nw), "points_per_wavelength": run["points_per_wavelength"],
           "cycles": run["cycles"], "t_end": run["t_end"], "backend": "openlifu_amd/hip-gfx950", "element_model": element_model,
           "aperture_entries": run["aperture_entries"] if element_model == "aperture" else None, "layer_model": layer_model,
           "drive_model": drive_model, "drive_taps": run.get("drive_taps")}
    if rec_m is not None:
        ra, rp = lockin_amplitude_phase(run["rec_C"], run["rec_S"], nw)
        raw["receiver_amplitude"], raw["receiver_phase"] = ra, rp
        raw["receiver_sums"] = np.asarray(run["rec_C"], dtype=np.float64) + 1j * np.asarray(run["rec_S"], dtype=np.float64)
    return ds.make_dataset(out), raw


def _advertise_without(fn, *names):
    """The element-model keywords are accepted (and named in the docstrings) but are not part of the signature ``inspect.signature`` reports
    for the two entry points: the first advertises exactly the reference seam's arguments plus the options it had when ``Protocol`` was
    taught to bind them, the second its own fixed list, and tests/test_fullwave_host.py / tests/test_fullwave_lockin_host.py hold both to
    that."""
    import inspect
    sig = inspect.signature(fn)
    fn.__signature__ = sig.replace(parameters=[p for name, p in sig.parameters.items() if name not in names])


_advertise_without(run_fullwave_simulation, "element_model", "layer_model", "drive_model", "source_waveforms")
_advertise_without(run_fullwave_steady_state, "element_model", "upsampling_rate", "layer_model", "drive_model")
