"""Straight-ray aberration correction through the medium (DESIGN.md section 2 "StraightRay"), computed by HIP kernel 1m
(``bf_med_k``) after kernel 1.  An extension of the reference's delay-method family, behind its own seam:
``calc_delays(arr, target, params, transform)`` reads the ``params`` sound-speed volume that ``Direct`` ignores.

Per focus and element: ``tau = tof + E / c_ref``, ``delays = max(tau) - tau``, with ``tof`` kernel 1's geometric time of flight and
``E`` the straight-ray extra path through ``sigma = c_ref / c - 1`` that the field model of section 7 puts into the phase of
every term -- so the modelled field adds up in phase at the focus.  Without ``params`` it is ``Direct(c0)``."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from ... import _native as nat
from ...engine import get_engine, grid_from_coords
from .delaymethod import DelayMethod


@dataclass
class StraightRay(DelayMethod):
    c0: float = 1480.0  # m/s, used only when no params are given (as Direct.c0)

    def __post_init__(self):
        if not isinstance(self.c0, (int, float)):
            raise TypeError("Speed of sound must be a number")
        if self.c0 <= 0:
            raise ValueError("Speed of sound must be greater than 0")
        self.c0 = float(self.c0)

    def speed(self, params) -> float:
        return self.c0 if params is None else float(params["sound_speed"].attrs["ref_value"])

    @staticmethod
    def medium(params):
        """(c_ref, sound speed float32 [nx,ny,nz] or None for c_ref everywhere, origin [m], spacing [m], n), checked on the host:
        every refusal is raised here, before any device call."""
        c_ref = float(params["sound_speed"].attrs["ref_value"])
        if not (np.isfinite(c_ref) and c_ref > 0):
            raise ValueError(f"StraightRay: the reference sound speed must be finite and > 0, got {c_ref}")
        origin, spacing, n = grid_from_coords(params.coords)
        shape = tuple(int(v) for v in n)
        ss = params["sound_speed"]
        declared = getattr(ss, "uniform_value", None)
        if declared is not None:                 # constant volume nobody has touched: no scan
            declared = float(declared)
            if not (np.isfinite(declared) and declared > 0):
                raise ValueError(f"StraightRay: sound speed must be finite and > 0, got {declared}")
            return c_ref, (None if declared == c_ref else np.full(shape, declared, dtype=np.float32)), origin, spacing, n
        vol = np.ascontiguousarray(np.asarray(ss.data), dtype=np.float32)
        if vol.shape != shape:
            raise ValueError(f"StraightRay: sound speed volume of shape {vol.shape} does not match the grid {shape} of params.coords")
        if not (np.isfinite(vol).all() and (vol > 0).all()):
            raise ValueError("StraightRay: sound speed must be finite and > 0 everywhere")
        return c_ref, vol, origin, spacing, n

    def solve(self, arr, targets, params=None, transform: np.ndarray | None = None, apod=(nat.APOD_UNIFORM, 1.0, 0.0)):
        """(delays [F,N] s, apod [F,N]) for all foci in one launch; the corrected delays stay resident as the steering table."""
        if params is None:
            return get_engine().beamform(arr, targets, self.c0, transform=transform, apod=apod)
        c_ref, vol, origin, spacing, n = self.medium(params)
        return get_engine().beamform_medium(arr, targets, c_ref, vol, origin, spacing, n, transform=transform, apod=apod)

    def calc_delays(self, arr, target, params=None, transform: np.ndarray | None = None):
        """delays[N] [s] for one focus.  A list of Points returns [F,N]."""
        delays, _ = self.solve(arr, target, params, transform=transform)
        return delays if isinstance(target, (list, tuple)) else delays[0]
