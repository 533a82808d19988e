"""Apodization that knows the medium (DESIGN.md section 2 "MediumCompensated"), computed by HIP kernel 1a (``bf_med_k<SIG, true>``)
after kernel 1.  An extension of the reference's apodization family, behind its own seam: ``calc_apodization(arr, target, params,
transform)`` reads the ``params`` attenuation volume that ``Uniform`` / ``MaxAngle`` / ``PiecewiseLinear`` ignore.

Per focus and element: ``h = exp(-A)`` (times ``S / max(d, dmin)`` with ``spreading``), ``A`` the straight-ray attenuation sum the field
model of section 7 puts into the amplitude of every term, ``b`` the base method's apodization, active = ``b > 0``:
``"equalize"``: ``b min_active(h) / h`` (equal arrival amplitudes), ``"matched"``: ``b h / max_active(h)`` (time-reversal amplitudes).
Without ``params`` it is its base method."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from ... import _native as nat
from ...engine import get_engine, grid_from_coords
from .apodmethod import ApodizationMethod
from .maxangle import MaxAngle
from .piecewiselinear import PiecewiseLinear
from .uniform import Uniform

BASES = (Uniform, MaxAngle, PiecewiseLinear)


@dataclass
class MediumCompensated(ApodizationMethod):
    base: ApodizationMethod = field(default_factory=Uniform)   # the geometric apodization b (kernel 1)
    mode: str = "equalize"
    spreading: bool = False          # also compensate the 1 / d spreading and the element areas
    frequency: float | None = None   # Hz; None: Protocol passes its pulse's

    def __post_init__(self):
        if isinstance(self.base, dict):
            self.base = ApodizationMethod.from_dict(self.base)
        if type(self.base) not in BASES:
            raise TypeError(f"Base must be one of {tuple(b.__name__ for b in BASES)}, got {type(self.base).__name__}")
        if self.mode not in nat.COMP_MODES:
            raise ValueError(f"Mode must be one of {tuple(nat.COMP_MODES)}, got {self.mode!r}")
        if not isinstance(self.spreading, (bool, np.bool_)):
            raise TypeError("Spreading must be a bool")
        self.spreading = bool(self.spreading)
        if self.frequency is not None:
            self.frequency = self.checked_frequency(self.frequency)

    @staticmethod
    def checked_frequency(frequency) -> float:
        if isinstance(frequency, bool) or not isinstance(frequency, (int, float)):
            raise TypeError("Frequency must be a number")
        if not (np.isfinite(frequency) and frequency > 0):
            raise ValueError(f"Frequency must be finite and greater than 0, got {frequency}")
        return float(frequency)

    def to_dict(self):
        return {"base": self.base.to_dict(), "mode": self.mode, "spreading": self.spreading, "frequency": self.frequency,
                "class": type(self).__name__}

    def kernel_args(self):
        """The base method's (apod_kind, p0, p1): what kernel 1 runs before kernel 1a."""
        return self.base.kernel_args()

    @staticmethod
    def medium(params):
        """(attenuation float32 [nx,ny,nz] in dB/cm/MHz^0.9 or None for none, origin [m], spacing [m], n), checked on the host: every
        refusal is raised here, before any device call."""
        origin, spacing, n = grid_from_coords(params.coords)
        shape = tuple(int(v) for v in n)
        att = params["attenuation"]
        declared = getattr(att, "uniform_value", None)
        if declared is not None:                 # constant volume nobody has touched: no scan
            declared = float(declared)
            if not (np.isfinite(declared) and declared >= 0):
                raise ValueError(f"MediumCompensated: attenuation must be finite and >= 0, got {declared}")
            return (None if declared == 0 else np.full(shape, declared, dtype=np.float32)), origin, spacing, n
        vol = np.ascontiguousarray(np.asarray(att.data), dtype=np.float32)
        if vol.shape != shape:
            raise ValueError(f"MediumCompensated: attenuation volume of shape {vol.shape} does not match the grid {shape} of params.coords")
        if not (np.isfinite(vol).all() and (vol >= 0).all()):
            raise ValueError("MediumCompensated: attenuation must be finite and >= 0 everywhere")
        return vol, origin, spacing, n

    def solve(self, arr, targets, params=None, transform: np.ndarray | None = None, frequency=None, delay_method=None):
        """(delays [F,N] s, apod [F,N]) for all foci in one launch; the table stays resident as the steering table.  ``frequency``
        [Hz] is used when the method has none of its own; ``delay_method``: ``Direct`` / ``StraightRay`` whose delays the table
        carries (None: kernel 1's at unit speed, as the other apodization methods solve) -- StraightRay's come from the same walk."""
        from ..delay_methods import StraightRay       # (the delay family does not import this one)
        if params is None:
            c = 1.0 if delay_method is None else delay_method.speed(None)
            return get_engine().beamform(arr, targets, c, transform=transform, apod=self.kernel_args())
        frequency = self.frequency if self.frequency is not None else frequency
        if frequency is None:
            raise ValueError("MediumCompensated: a frequency is needed to read the attenuation of params (set `frequency`, or solve through a Protocol)")
        frequency = self.checked_frequency(frequency)
        att, origin, spacing, n = self.medium(params)
        sound_speed, c = False, 1.0
        if type(delay_method) is StraightRay:
            c, sound_speed, _, _, _ = StraightRay.medium(params)
        elif delay_method is not None:
            c = delay_method.speed(params)
        return get_engine().beamform_compensated(arr, targets, c, att, origin, spacing, n, frequency, transform=transform,
                                                 apod=self.kernel_args(), mode=self.mode, spreading=self.spreading, sound_speed=sound_speed)

    def calc_apodization(self, arr, target, params=None, transform=None):
        """weights[N] for one focus.  A list of Points returns [F,N]."""
        _, apod = self.solve(arr, target, params, transform=transform)
        return apod if isinstance(target, (list, tuple)) else apod[0]
