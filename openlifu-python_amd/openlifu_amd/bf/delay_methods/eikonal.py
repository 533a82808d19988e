"""Eikonal delays: refracted first-arrival travel times through the medium (DESIGN.md section 2 "Eikonal", HIP kernel 6, section 5.17).
Between ``StraightRay`` (microseconds, no refraction) and ``TimeReversal`` (one full-wave run per focus, seconds): per focus TWO eikonal
solves from the target -- ``T_med`` through the ``params`` sound speed, ``T_ref`` through ``c_ref`` everywhere -- read at the elements by
reciprocity (trilinear, the rule of ``sim/fullwave.py::trilinear_entries``).  Only their DIFFERENCE is used: the first-order scheme's
error around a point source is larger than the refraction it is after, and cancels in the difference.

Per focus and element: ``E = c_ref (T_med - T_ref)`` [m], ``tau = |x_e - x_t| / c_ref + E / c_ref``, ``delays = max(tau) - tau`` --
``StraightRay``'s form with the extra path taken along the refracted first arrival.  Without ``params`` it is ``Direct(c0)``; with a
medium that is ``c_ref`` everywhere no solve runs and the delays are kernel 1's."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from ...engine import focus_positions_m, get_engine
from .delaymethod import DelayMethod
from .straightray import StraightRay


def source_index(target_m, origin_m, spacing_m, n, focus: int = 0):
    """Index coordinates q of a target on the grid; ValueError naming the target unless 0 <= q_a <= n_a - 1 on every axis."""
    t = np.asarray(target_m, dtype=np.float64)
    q = (t - np.asarray(origin_m, dtype=np.float64)) / np.asarray(spacing_m, dtype=np.float64)
    if not (np.all(np.isfinite(q)) and np.all(q >= 0) and np.all(q <= np.asarray(n, dtype=np.float64) - 1)):
        raise ValueError(f"Eikonal: target {focus} at {tuple(float(v) for v in t)} m does not lie inside the grid "
                         f"(index coordinates {tuple(float(v) for v in q)}, grid {tuple(int(v) for v in n)})")
    return q


@dataclass
class Eikonal(DelayMethod):
    c0: float = 1480.0  # m/s, used only when no params are given (as Direct.c0)
    init_radius: float = 3.0            # voxels: the ball around the target that starts at the analytic time
    max_sweeps: int | None = None       # None: 4 (nx + ny + nz)

    def __post_init__(self):
        if isinstance(self.c0, bool) or not isinstance(self.c0, (int, float)):
            raise TypeError("Speed of sound must be a number")
        if self.c0 <= 0:
            raise ValueError("Speed of sound must be greater than 0")
        self.c0 = float(self.c0)
        r = self.init_radius
        if isinstance(r, bool) or not isinstance(r, (int, float)):
            raise TypeError("Eikonal: init_radius must be a number")
        if not (np.isfinite(r) and r >= 1):
            raise ValueError(f"Eikonal: init_radius must be finite and >= 1, got {r!r}")
        self.init_radius = float(r)
        if self.max_sweeps is not None:
            m = self.max_sweeps
            if isinstance(m, bool) or not isinstance(m, (int, np.integer)):
                raise TypeError("Eikonal: max_sweeps must be an integer or None")
            if m < 1:
                raise ValueError(f"Eikonal: max_sweeps must be >= 1, got {m!r}")
            self.max_sweeps = int(m)

    def speed(self, params) -> float:
        return self.c0 if params is None else float(params["sound_speed"].attrs["ref_value"])

    def solve(self, arr, targets, params=None, transform: np.ndarray | None = None, return_volumes: bool = False):
        """(delays [F,N] s, info) -- two eikonal solves per focus.  ``info`` holds per focus ``extra_path_m`` [N], ``travel_time_s`` [N]
        (tau), ``sweeps`` = (medium, reference) and, with ``return_volumes``, ``volumes`` = (T_med, T_ref) float32 [nx, ny, nz]."""
        info = {"extra_path_m": [], "travel_time_s": [], "sweeps": []}
        if return_volumes:
            info["volumes"] = []
        if params is None:
            return get_engine().beamform(arr, targets, self.c0, transform=transform)[0], info
        c_ref, vol, origin, spacing, n = StraightRay.medium(params)
        if vol is None:             # c_ref everywhere: no refraction, no solve -- kernel 1's delays
            return get_engine().beamform(arr, targets, c_ref, transform=transform)[0], info
        from ...sim.fullwave import receiver_table      # (sim imports bf through plan: resolve at call time)
        foci = focus_positions_m(targets)
        if foci.ndim != 2 or foci.shape[1] != 3:
            raise ValueError(f"targets must give positions of shape (F, 3), got {foci.shape}")
        pos = np.asarray(arr.element_table()[0], dtype=np.float64)
        if transform is not None:
            M = np.asarray(transform, dtype=np.float64)
            if M.shape != (4, 4):
                raise ValueError(f"transform must be a 4 x 4 matrix, got {M.shape}")
            pos = pos @ M[:3, :3].T + M[:3, 3]
        # every refusal before a device call: the targets, then the elements' trilinear voxels
        for f in range(foci.shape[0]):
            source_index(foci[f], origin, spacing, n, f)
        try:
            row, ijk, wt = receiver_table(pos, origin, spacing, n)
        except ValueError as e:
            raise ValueError(str(e).replace("full-wave simulation: receiver", "Eikonal: element")) from None
        lin = (ijk[:, 0] * int(n[1]) + ijk[:, 1]) * int(n[2]) + ijk[:, 2]
        table = (row, lin, wt)
        eng = get_engine()
        delays = np.empty((foci.shape[0], pos.shape[0]))
        for f in range(foci.shape[0]):
            t_med, s_med, v_med = eng.eikonal(origin, spacing, n, vol, foci[f], table, self.init_radius, self.max_sweeps, volume=return_volumes)
            t_ref, s_ref, v_ref = eng.eikonal(origin, spacing, n, c_ref, foci[f], table, self.init_radius, self.max_sweeps, volume=return_volumes)
            extra = c_ref * (t_med - t_ref)
            tau = np.sqrt(((pos - foci[f]) ** 2).sum(axis=1)) / c_ref + extra / c_ref
            delays[f] = tau.max() - tau
            info["extra_path_m"].append(extra); info["travel_time_s"].append(tau); info["sweeps"].append((s_med, s_ref))
            if return_volumes:
                info["volumes"].append((v_med, v_ref))
        return delays, info

    def calc_delays(self, arr, target, params=None, transform: np.ndarray | None = None):
        """delays[N] [s] for one focus.  A list of Points returns [F,N]."""
        delays = self.solve(arr, target, params, transform=transform)[0]
        return delays if isinstance(target, (list, tuple)) else delays[0]
