"""Time-reversal delays from the full-wave model (DESIGN.md section 2 "TimeReversal", HIP kernel 5 with its lock-in, section 5.15): a
monopole at the target radiates through the ``params`` medium, the elements listen, and the array fires the conjugate.  Refraction and
the reflection / transmission at interfaces, which the ray rules ``Direct`` and ``StraightRay`` leave out, are in the delays.

Per focus ONE driven full-wave run (cost: section 5.14's table, a whole run per focus -- seconds where ``StraightRay`` takes
microseconds).  The run gives each element the steady-state sum Z_e = C_e + i S_e at the drive frequency f0, hence the lag psi_e
[cycles, (-1/2, 1/2]] of the received wave: its travel time T_e is (psi_e + m_e) / f0 with an unknown whole number m_e.  A ray rule
(the ``anchor``: ``StraightRay``, or ``Direct``) is good to well within half a cycle, so it fixes m_e: with the anchor's relative
delays d_e, x_e = -f0 d_e - psi_e, off = the |Z_e|-weighted circular mean of x_e (the common travel time that relative delays do not
know), m_e = rint(x_e - off), T_e = (psi_e + m_e) / f0 and delays_e = max T - T_e.  The tie margin 1/2 - max |x_e - off - m_e| says how
far the rounding was from a wrap; below ``TIE_WARN`` a warning is logged.  Without ``params`` it is ``Direct(c0)``.

``element_model="point"`` (the default) samples p trilinearly at each element's centre; ``"aperture"`` makes Z_e the average of p over
the element's rectangle (``upsampling_rate`` quadrature points per smallest voxel edge, DESIGN.md section 2 "full-wave model:
apertures"), so an element a wavelength wide hears an oblique wave with its directivity, in amplitude and in phase.
``layer_model="pml"`` runs the listening run with split perfectly matched layers in place of the sponge (DESIGN.md section 2 "full-wave
model: split layers"): the choice for a grid cropped narrowly around the beam."""
from __future__ import annotations

import logging
from dataclasses import dataclass

import numpy as np

from ...engine import focus_positions_m, get_engine
from .delaymethod import DelayMethod
from .straightray import StraightRay

ANCHORS = ("straight_ray", "direct")
TIE_WARN = 0.05     # cycles


def unwrap_against_anchor(Z, anchor_delays, frequency):
    """(delays [N] s, tie margin [cycles], m [N]) from the received sums Z_e = C_e + i S_e and the anchor's relative delays [s]."""
    Z = np.asarray(Z, dtype=np.complex128)
    d = np.asarray(anchor_delays, dtype=np.float64)
    f0 = float(frequency)
    psi = np.arctan2(-Z.real, Z.imag) / (2.0 * np.pi)
    psi = np.where(psi <= -0.5, 0.5, psi)
    x = -f0 * d - psi
    off = np.angle(np.sum(np.abs(Z) * np.exp(2j * np.pi * x))) / (2.0 * np.pi)
    m = np.rint(x - off)
    T = (psi + m) / f0
    return T.max() - T, float(0.5 - np.abs(x - off - m).max()), m.astype(np.int64)


@dataclass
class TimeReversal(DelayMethod):
    c0: float = 1480.0  # m/s, used only when no params are given (as Direct.c0)
    frequency: float | None = None   # Hz; None: Protocol passes its pulse's
    lockin_cycles: float = 4
    settle_cycles: float = 3
    ramp_cycles: float = 2.0
    cfl: float = 0.3
    pml_size: int = 16
    anchor: str = "straight_ray"
    element_model: str = "point"     # "aperture": the elements listen with the averages over their rectangles (sim/fullwave.py)
    upsampling_rate: int = 5         # quadrature points per smallest voxel edge of the "aperture" model
    layer_model: str = "sponge"      # "pml": the run's absorbing layers are split perfectly matched layers (sim/fullwave.py)

    def __post_init__(self):
        if isinstance(self.c0, bool) or not isinstance(self.c0, (int, float)):
            raise TypeError("Speed of sound must be a number")
        if self.c0 <= 0:
            raise ValueError("Speed of sound must be greater than 0")
        self.c0 = float(self.c0)
        if self.frequency is not None:
            self.frequency = self.checked_frequency(self.frequency)
        for name in ("lockin_cycles", "settle_cycles", "ramp_cycles", "cfl"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not np.isfinite(v) or v < 0:
                raise ValueError(f"TimeReversal: {name} must be a finite number >= 0, got {v!r}")
        if not (self.lockin_cycles > 0 and self.cfl > 0):
            raise ValueError("TimeReversal: lockin_cycles and cfl must be greater than 0")
        if isinstance(self.pml_size, bool) or not isinstance(self.pml_size, (int, np.integer)) or self.pml_size < 0:
            raise ValueError(f"TimeReversal: pml_size must be an integer >= 0, got {self.pml_size!r}")
        self.pml_size = int(self.pml_size)
        if self.anchor not in ANCHORS:
            raise ValueError(f"TimeReversal: anchor must be one of {ANCHORS}, got {self.anchor!r}")
        from ...sim.fullwave import checked_element_model, checked_layer_model      # (sim imports bf through plan: resolve at call time)
        self.element_model, self.upsampling_rate = checked_element_model(self.element_model, self.upsampling_rate)
        self.layer_model = checked_layer_model(self.layer_model)

    def to_dict(self):
        """The tagged dict; the element model and the layer model are written only when they are not the defaults, so the stored form of a
        method that does not use them is what it was before the options existed (``from_dict`` fills the defaults in)."""
        d = super().to_dict()
        if self.element_model == "point":
            del d["element_model"], d["upsampling_rate"]
        if self.layer_model == "sponge":
            del d["layer_model"]
        return d

    @staticmethod
    def checked_frequency(frequency) -> float:
        if isinstance(frequency, bool) or not isinstance(frequency, (int, float)):
            raise TypeError("Frequency must be a number")
        if not (np.isfinite(frequency) and frequency > 0):
            raise ValueError(f"Frequency must be finite and greater than 0, got {frequency}")
        return float(frequency)

    def speed(self, params) -> float:
        return self.c0 if params is None else float(params["sound_speed"].attrs["ref_value"])

    def solve(self, arr, targets, params=None, transform: np.ndarray | None = None, frequency=None):
        """(delays [F,N] s, amplitudes [F,N] = 2 / Nw |Z_e| [Pa per unit monopole], info) -- one full-wave run per focus.  ``info`` holds
        per focus the tie margin [cycles], the whole cycles m_e and the run's ``raw``.  ``frequency`` is used when the method has none."""
        if params is None:
            delays, _ = get_engine().beamform(arr, targets, self.c0, transform=transform)
            return delays, np.ones_like(delays), {"tie_margin": [], "cycles": [], "raw": []}
        frequency = self.frequency if self.frequency is not None else frequency
        if frequency is None:
            raise ValueError("TimeReversal: a frequency is needed to drive the full-wave run (set `frequency`, or solve through a Protocol)")
        frequency = self.checked_frequency(frequency)
        from ...sim.fullwave import aperture_geometry, lockin_amplitude_phase, steady_state_run      # (sim imports bf through plan: resolve at call time)
        from ...engine import grid_from_coords
        foci = focus_positions_m(targets)
        pos = np.asarray(arr.element_table()[0], dtype=np.float64)
        if transform is not None:
            M = np.asarray(transform, dtype=np.float64)
            if M.shape != (4, 4):
                raise ValueError(f"transform must be a 4 x 4 matrix, got {M.shape}")
            pos = pos @ M[:3, :3].T + M[:3, 3]
        listen = {"receivers_m": pos}
        if self.element_model == "aperture":      # Z_e is the average of p over the element's rectangle: sum_m W_e(m) p(m)
            listen = {"receiver_apertures": aperture_geometry(arr, grid_from_coords(params.coords)[1], self.upsampling_rate, transform=transform)}
        if self.layer_model != "sponge":
            listen["layer_model"] = self.layer_model
        runs = []
        for f in range(foci.shape[0]):
            runs.append(steady_state_run(params, foci[f][None], [1.0], [0.0], frequency, cfl=self.cfl, lockin_cycles=self.lockin_cycles,
                                         settle_cycles=self.settle_cycles, ramp_cycles=self.ramp_cycles, pml_size=self.pml_size, volume=False,
                                         what="target", **listen))
        if self.anchor == "straight_ray":
            anchor = StraightRay(c0=self.c0).solve(arr, foci, params, transform=transform)[0]
        else:
            anchor = get_engine().beamform(arr, foci, self.speed(params), transform=transform)[0]
        delays, amps, info = np.empty((foci.shape[0], pos.shape[0])), np.empty((foci.shape[0], pos.shape[0])), {"tie_margin": [], "cycles": [], "raw": []}
        for f, run in enumerate(runs):
            Z = np.asarray(run["rec_C"]) + 1j * np.asarray(run["rec_S"])
            delays[f], margin, m = unwrap_against_anchor(Z, anchor[f], frequency)
            amps[f] = lockin_amplitude_phase(Z.real, Z.imag, run["window"][1])[0]
            if margin < TIE_WARN:
                logging.getLogger(__name__).warning("TimeReversal: focus %d: tie margin %.3f cycles is below %g: an element's whole cycle "
                                                    "may be off by one (the anchor and the received phase disagree by almost half a cycle)", f, margin, TIE_WARN)
            info["tie_margin"].append(margin); info["cycles"].append(m)
            info["raw"].append({"dt": run["dt"], "n_steps": run["n_steps"], "window": run["window"], "points_per_wavelength": run["points_per_wavelength"],
                                "receiver_sums": Z, "backend": "openlifu_amd/hip-gfx950"})
        return delays, amps, info

    def calc_delays(self, arr, target, params=None, transform: np.ndarray | None = None, frequency=None):
        """delays[N] [s] for one focus.  A list of Points returns [F,N]."""
        delays = self.solve(arr, target, params, transform=transform, frequency=frequency)[0]
        return delays if isinstance(target, (list, tuple)) else delays[0]
