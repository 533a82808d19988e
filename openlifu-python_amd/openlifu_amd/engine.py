"""Host-side driver of the device hot path: one ``Engine`` per GPU owns a native
context (include/olx.h), keeps the transducer's element table resident and turns
the reference's per-focus Python calls into batched launches.

There is no CPU path here: every method ends in a HIP kernel launched through
the C-ABI, and raises if the library or the GPU is missing.
"""
from __future__ import annotations

import os
import weakref

import numpy as np

from . import _native as nat
from .geo import Point
from .util.units import getunitconversion

_engines: dict[int, "Engine"] = {}


def default_device() -> int:
    for var in ("OPENLIFU_AMD_DEVICE", "LOCAL_RANK"):
        if os.environ.get(var, "") != "":
            return int(os.environ[var])
    return 0


def get_engine(device: int | None = None) -> "Engine":
    device = default_device() if device is None else int(device)
    if device not in _engines:
        _engines[device] = Engine(device)
    return _engines[device]


def gpu_available() -> bool:
    """HIP probe standing in for openlifu.util.checkgpu.gpu_available (NVML-only in the
    reference, util/checkgpu.py:6-14, hence always False on AMD)."""
    try:
        return nat.device_count() > 0
    except Exception:  # noqa: BLE001 - same contract as the reference: any failure = no GPU
        return False


PULSE_C_GRID = 1500.0     # the sound speed of the time-axis defaults (get_kgrid's makeTime(1500, cfl))


def pulse_time_axis(spacing_m, n, dt: float = 0.0, t_end: float = 0.0, cfl: float = 0.5):
    """(dt [s], n_t) of the pulsed model's time axis t_k = k dt, k < n_t.  ``dt > 0`` is used as given, ``dt == 0``
    gives cfl min(spacing) / 1500; ``t_end > 0`` gives n_t = floor(t_end / dt) + 1, ``t_end == 0`` uses t_end = |(nx, ny, nz) spacing| / 1500.
    The two defaults are this project's contract, written after get_kgrid's makeTime(1500, cfl) as SURVEY.md records it."""
    spacing = np.broadcast_to(np.asarray(spacing_m, dtype=np.float64), (3,))
    n = np.asarray(n, dtype=np.float64)
    dt, t_end, cfl = float(dt), float(t_end), float(cfl)
    if not (np.isfinite(dt) and dt >= 0 and np.isfinite(t_end) and t_end >= 0):
        raise ValueError(f"dt and t_end must be finite and >= 0 (0 = default), got dt={dt}, t_end={t_end}")
    if dt == 0:
        if not (np.isfinite(cfl) and cfl > 0):
            raise ValueError(f"the default dt needs cfl > 0, got {cfl}")
        dt = cfl * float(spacing.min()) / PULSE_C_GRID
    if t_end == 0:
        t_end = float(np.sqrt(np.sum((n * spacing) ** 2))) / PULSE_C_GRID
    n_t = int(np.floor(t_end / dt)) + 1
    if n_t >= 2 ** 31:
        raise ValueError(f"time axis of {n_t} samples is too long")
    return dt, n_t


def focus_positions_m(targets) -> np.ndarray:
    """[F,3] metres from a Point, a list of Points, or an array already in metres."""
    if isinstance(targets, Point):
        targets = [targets]
    if isinstance(targets, (list, tuple)) and len(targets) and isinstance(targets[0], Point):
        return np.array([t.get_position(units="m") for t in targets], dtype=np.float64)
    return np.atleast_2d(np.asarray(targets, dtype=np.float64))


class DeviceResult:
    """Handle on the F focus volumes one launch left resident in HBM (``Engine.field(..., lazy=True)``).  ``fetch(key)``
    returns a fresh [F, nx, ny, nz] float32 array while the engine still holds this result; before the engine
    overwrites its buffers (next launch / upload) it calls ``retire()``, which brings every array that was handed out
    lazily and not read yet to the host, so outstanding ``LazyDataArray``s stay valid."""

    def __init__(self, engine, n_foci, shape, keys):
        self.engine, self.token = engine, engine.result_token
        self.shape = (int(n_foci),) + tuple(int(v) for v in shape)
        self.keys = tuple(keys)
        self._lazies = []        # weak references to the LazyDataArrays fed by this result
        self.retired = False

    def fetch(self, key):
        if self.retired or self.engine.result_token != self.token:
            raise RuntimeError("the device result this array belongs to has been overwritten")
        return self.engine.ctx.field_fetch_all(want=(key,))[key]

    def lazy_array(self, key, make):
        """``make(fetch)`` builds the LazyDataArray; it is remembered (weakly) for ``retire``."""
        da = make(lambda: self.fetch(key))
        self._lazies.append(weakref.ref(da))
        return da

    def retire(self):
        if self.retired:
            return
        for ref in self._lazies:
            da = ref()
            if da is not None and not da.materialized:
                _ = da.data          # fetch now: the buffers are about to be reused
        self.retired = True


class AggregateResult:
    """Handle on the aggregate over foci (max |p|, mean intensity: plan/protocol.py:382-387) that ``Engine.aggregate_lazy``
    left in HBM.  ``fetch(key)`` returns a fresh [nx, ny, nz] float32 array while the aggregate buffers still hold this
    result; ``retire()`` (called by the engine before the buffers are reused) reads every lazily handed-out array nobody
    has read yet, so outstanding ``LazyDataArray``s stay valid -- and an aggregate nobody looks at costs no PCIe traffic."""

    def __init__(self, engine, shape):
        self.engine, self.shape = engine, tuple(int(v) for v in shape)
        self.pulsed = bool(getattr(engine, "_pmax_resident", False))   # pulsed volumes: p_max is aggregated apart ("pmax")
        self._lazies = []
        self.retired = False

    def fetch(self, key):
        if self.retired:
            raise RuntimeError("the device aggregate this array belongs to has been overwritten")
        if key == "pmax":       # pulsed plans: max_f p_max_f
            return self.engine.ctx.aggregate_fetch_pmax()
        pm, it = self.engine.ctx.aggregate_fetch(want_intensity=(key == "intensity"), want_pmag=(key == "pmag"))
        return pm if key == "pmag" else it

    def lazy_array(self, key, make):
        da = make(lambda: self.fetch(key))
        self._lazies.append(weakref.ref(da))
        return da

    def retire(self):
        if self.retired:
            return
        for ref in self._lazies:
            da = ref()
            if da is not None and not da.materialized:
                _ = da.data
        self.retired = True


class WeightedResult:
    """Handle on the time-average intensity volume (``Solution.get_ita``, plan/solution.py:365-388) that ``Engine.weighted_lazy`` left in
    HBM; same contract as ``AggregateResult``: ``retire()`` reads a lazily handed-out array nobody has read yet before the buffer is rewritten."""

    def __init__(self, engine, shape):
        self.engine, self.shape = engine, tuple(int(v) for v in shape)
        self._lazies = []
        self.retired = False

    def fetch(self):
        if self.retired:
            raise RuntimeError("the device volume this array belongs to has been overwritten")
        return self.engine.ctx.field_weighted_fetch()

    def lazy_array(self, make):
        da = make(self.fetch)
        self._lazies.append(weakref.ref(da))
        return da

    def retire(self):
        if self.retired:
            return
        for ref in self._lazies:
            da = ref()
            if da is not None and not da.materialized:
                _ = da.data
        self.retired = True


class PiiVolumeResult:
    """Handle on one volume ``Engine.pii_post`` left in HBM: ``which`` = "max" (max_f PII_f) or "weighted" (sum_f w_f PII_f); same contract
    as ``WeightedResult``: ``retire()`` reads a lazily handed-out array nobody has read yet before the buffer is rewritten."""

    def __init__(self, engine, shape, which):
        self.engine, self.shape, self.which = engine, tuple(int(v) for v in shape), which
        self._lazies = []
        self.retired = False

    def fetch(self):
        if self.retired:
            raise RuntimeError("the device volume this array belongs to has been overwritten")
        return self.engine.ctx.pii_fetch_max() if self.which == "max" else self.engine.ctx.pii_fetch_weighted()

    def lazy_array(self, make):
        da = make(self.fetch)
        self._lazies.append(weakref.ref(da))
        return da

    def retire(self):
        if self.retired:
            return
        for ref in self._lazies:
            da = ref()
            if da is not None and not da.materialized:
                _ = da.data
        self.retired = True


class Engine:
    def __init__(self, device: int = 0):
        self.ctx = nat.Context(device)
        self.device = device
        self._table_key = None
        self.result_token = 0  # bumped whenever the resident result volumes change
        self._live_result = None
        self._live_aggregate = None
        # every path that rewrites the aggregate buffers -- ctx.field_aggregate, the cross-rank all-reduce / reduce-scatter of
        # dist.ShardedField, another aggregate_lazy -- first brings a lazily handed-out aggregate Dataset to the host
        self.ctx.before_aggregate = self._retire_aggregate
        self._live_weighted = None
        self.ctx.before_weighted = self._retire_weighted      # (field_weighted_intensity and solution_analyze rewrite the time-average volume)
        self._live_pii = []            # PiiVolumeResults of the last pii_post
        self._pii_token = -1           # the result_token the resident PII volumes belong to (pii_resident)
        self.ctx.before_pii = self._retire_pii

    def _retire_pii(self):
        live, self._live_pii = self._live_pii, []
        for h in live:
            h.retire()

    def pii_resident(self) -> bool:
        """The device holds PII volumes that belong to the resident result (a pulsed launch with "pii", or ``upload_pii`` since)."""
        return self._pii_token == self.result_token

    def pii_post(self, n_foci, scale=None, weights=None, frames=None, **masks):
        """``ctx.pii_post`` over the resident PII -> (peaks | None, {"max": handle, "weighted": handle | absent}): lazy handles on the
        volumes it left in HBM (those of an earlier call are read to the host first where somebody still holds them unread)."""
        if not self.pii_resident():
            raise RuntimeError("no pulse intensity integrals resident for the current device result")
        peaks = self.ctx.pii_post(n_foci, scale=scale, weights=weights, A=frames, **masks)      # (retires the live handles through the hook)
        vols = {"max": PiiVolumeResult(self, self.ctx._shape, "max")}
        if weights is not None:
            vols["weighted"] = PiiVolumeResult(self, self.ctx._shape, "weighted")
        self._live_pii = list(vols.values())
        return peaks, vols

    def upload_pii(self, pii):
        """Host PII volumes [F, nx, ny, nz] become the resident PII of the current device result."""
        self.ctx.pii_upload(pii)
        self._pii_token = self.result_token

    def _retire_weighted(self):
        if self._live_weighted is not None:
            live, self._live_weighted = self._live_weighted, None
            live.retire()

    def _retire_aggregate(self):
        if self._live_aggregate is not None:
            live, self._live_aggregate = self._live_aggregate, None
            live.retire()

    def retire_results(self):
        """Call before anything overwrites the resident volumes: outstanding lazy arrays are brought to the host."""
        if self._live_aggregate is not None:      # (a plan / upload that needs larger volumes frees the aggregate buffers too)
            self._live_aggregate.retire()
            self._live_aggregate = None
        self._retire_weighted()
        self._retire_pii()
        if self._live_result is not None:
            self._live_result.retire()
            self._live_result = None

    def aggregate_lazy(self, want_intensity=True) -> AggregateResult:
        """Aggregate the resident focus volumes on the device and return the handle its lazy arrays fetch through."""
        self.ctx.field_aggregate_device(want_intensity=want_intensity)      # (retires a live aggregate through the hook)
        self._live_aggregate = AggregateResult(self, self.ctx._shape)
        return self._live_aggregate

    def scale_aggregate_lazy(self, factors) -> AggregateResult:
        """Per-focus scaling of the resident volumes AND their aggregate in one pass over HBM (``olx_field_scale_aggregate``:
        the values of ``ctx.field_scale`` followed by ``aggregate_lazy``)."""
        self.ctx.field_scale_aggregate(factors)                              # (retires a live aggregate through the hook)
        self._live_aggregate = AggregateResult(self, self.ctx._shape)
        return self._live_aggregate

    def weighted_lazy(self, weights) -> WeightedResult:
        """max_f weights[f] intensity_f over the resident focus volumes, left in HBM: the single "time-average" volume ``Solution.analyze``'s
        masked maxima scan (the reference takes them over the whole [focus, x, y, z] stack of ``get_ita``, plan/solution.py:243, 274).  The
        kernels keep their round-1 names (``field_weighted_sum_k`` / ``_peak_k``); rounds 1-4 formed the count-weighted SUM here."""
        self.ctx.field_weighted_intensity(weights)                           # (retires a live one through the hook)
        self._live_weighted = WeightedResult(self, self.ctx._shape)
        return self._live_weighted

    def adopt_aggregate(self) -> AggregateResult:
        """Handle on the aggregate a fused device call (``ctx.solution_analyze(..., scale=...)``) just left in the aggregate buffers."""
        self._live_aggregate = AggregateResult(self, self.ctx._shape)
        return self._live_aggregate

    # ---- element table ----------------------------------------------------------------------
    @staticmethod
    def _table_of(arr):
        """(pos, nrm, area * sensitivity, key): ``arr``'s SoA element table as the device takes it, and its hash."""
        cached = getattr(arr, "_cached", None)
        return cached("engine_table", lambda: Engine._table_of_now(arr)) if cached is not None else Engine._table_of_now(arr)

    @staticmethod
    def _table_of_now(arr):
        pos, nrm, area, _, _ = arr.element_table()
        # per-element sensitivity factors (Transducer.merge, xdc/transducer.py:236-247) scale the
        # element's drive exactly like its area does in the source weight
        sens = np.array([1.0 if el.sensitivity is None else el.sensitivity for el in arr.elements])
        area = area * sens
        return pos, nrm, area, hash((pos.tobytes(), nrm.tobytes(), area.tobytes()))

    def bind(self, arr):
        """Upload ``arr``'s SoA element table unless the resident one is identical."""
        pos, nrm, area, key = self._table_of(arr)
        if key != self._table_key:
            self.ctx.set_elements(pos, nrm, area)
            self._table_key = key
        return self.ctx.n_el

    # ---- kernel 1 -----------------------------------------------------------------------------
    def beamform(self, arr, targets, c: float, transform=None, apod=(nat.APOD_UNIFORM, 1.0, 0.0)):
        """delays[F,N] (s), apod[F,N] for F foci in ONE launch (replaces F x N Python calls,
        plan/protocol.py:318-320 -> bf/delay_methods/direct.py:35, bf/apod_methods/maxangle.py:36)."""
        self.bind(arr)
        kind, p0, p1 = apod
        return self.ctx.bf_solve(focus_positions_m(targets), c, matrix=transform, apod_kind=kind, p0=p0, p1=p1)

    # ---- kernel 1m ----------------------------------------------------------------------------
    def beamform_medium(self, arr, targets, c_ref: float, sound_speed, origin_m, spacing_m, n, transform=None,
                        apod=(nat.APOD_UNIFORM, 1.0, 0.0)):
        """StraightRay delays[F,N] (s) through the sound-speed volume (None = c_ref everywhere) and kernel 1's apod[F,N]: the medium is
        uploaded once, all foci are solved in one launch and the corrected table stays resident as the steering table.  The field
        plan, its medium and its volumes are left as they are."""
        self.bind(arr)
        kind, p0, p1 = apod
        self.ctx.bf_set_medium(sound_speed, origin_m, spacing_m, n, c_ref)
        return self.ctx.bf_solve_medium(focus_positions_m(targets), c_ref, matrix=transform, apod_kind=kind, p0=p0, p1=p1)

    # ---- kernel 1a (alone, or in one walk with 1m) ----------------------------------------------
    def beamform_compensated(self, arr, targets, c: float, attenuation, origin_m, spacing_m, n, freq_hz: float, transform=None,
                             apod=(nat.APOD_UNIFORM, 1.0, 0.0), mode="equalize", spreading=False, sound_speed=False):
        """delays[F,N] (s) and the MediumCompensated apod[F,N] through the attenuation volume (dB/cm/MHz^0.9, None = none) at ``freq_hz``;
        ``apod`` is the base method's kernel-1 arguments.  ``sound_speed`` other than False (a volume, or None = c everywhere) also
        corrects the delays as ``beamform_medium`` does (c = the reference speed), by the same walk of the rays.  The table stays
        resident as the steering table; the field plan, its medium and its volumes are left as they are."""
        self.bind(arr)
        kind, p0, p1 = apod
        with_delays = sound_speed is not False
        if with_delays:
            self.ctx.bf_set_medium(sound_speed, origin_m, spacing_m, n, c)
        self.ctx.bf_set_attenuation(attenuation, origin_m, spacing_m, n, freq_hz)
        return self.ctx.bf_solve_compensated(focus_positions_m(targets), c, matrix=transform, apod_kind=kind, p0=p0, p1=p1, mode=mode,
                                             spreading=spreading, use_delay_medium=with_delays)

    # ---- kernel 2 -----------------------------------------------------------------------------
    def field(self, arr, delays, apod, origin_m, spacing_m, n, freq, c, rho, p0_pa,
              want=("pmag", "intensity"), slab=None, steering_resident=False, medium=None, fp8_correction=None,
              lazy=False, directivity=False, absorption=0.0, pulse=None, trace_voxels=None, pulsed_medium_model=None,
              pulsed_drive_model=None):
        """Pressure field for F foci -> dict of float32 arrays [F, nx, ny, nz] (fresh, writable,
        caller-owned).  ``steering_resident`` reuses the table the last ``beamform`` left on the
        device instead of uploading ``delays`` / ``apod``.  ``fp8_correction=False`` opts OUT of the e4m3
        correction products the lattice kernels use by default where their bound (<= 7.5e-6 of the volume maximum, include/olx.h) is a bound on the
        planned volume (include/olx.h OLX_FIELD_FP16_CORRECTION: three fp16 products everywhere, <= 2e-6).  ``directivity`` opts in to the far-field piston factor of the elements
        (OLX_FIELD_DIRECTIVITY; folded into the lattice kernels' tables for flat arrays of equal axis-aligned elements, else the exact
        per-pair kernel; homogeneous media).  ``absorption`` [Np/m] > 0: uniform absorbing medium, every term carries exp(-a d)
        (olx_field_absorption).  ``lazy=True`` returns a ``DeviceResult`` instead: the volumes
        stay in HBM until somebody reads them.  ``pulse = (cycles, dt, t_end, cfl)`` selects the pulsed model (olx_field_pulse, time axis by
        ``pulse_time_axis``): "pmag" then holds p_min and the result carries p_max under "pmax"; "pii" in ``want`` adds the pulse
        intensity integral [J/cm^2] (OLX_OUT_PII; a lazy result carries it like p_max, under "pii"), ``trace_voxels`` (linear voxel indices) adds the waveforms
        p(t_k) there under "trace" [F, P, n_t] (olx_field_pulse_trace).  ``pulsed_medium_model="straight_ray"`` lets the pulsed model take a
        ``medium`` (olx_field_pulse_medium, kernel 2ph); without it a pulsed request with a medium is refused.
        ``pulsed_drive_model="impulse_response"`` drives the pulsed model through ``arr``'s impulse responses (sim/field.py ``drive_taps`` at the
        plan's dt, olx_field_pulse_response; no medium); an array without any response runs the plain kernel."""
        if pulsed_drive_model not in (None, "impulse_response"):
            raise ValueError(f'pulsed_drive_model must be None or "impulse_response", got {pulsed_drive_model!r}')
        if pulsed_drive_model is not None and pulse is None:
            raise ValueError("pulsed_drive_model needs the pulsed field model (the continuous-wave model has no drive waveform)")
        if pulsed_medium_model not in (None, "straight_ray"):
            raise ValueError(f'pulsed_medium_model must be None or "straight_ray", got {pulsed_medium_model!r}')
        if pulsed_medium_model is not None and pulse is None:
            raise ValueError("pulsed_medium_model needs the pulsed field model (the continuous-wave model picks its medium kernels by itself)")
        if pulse is None and ("pii" in want or trace_voxels is not None):
            raise ValueError('the pulse intensity integral ("pii") and the waveform traces need the pulsed field model')
        if pulse is not None:
            if medium is not None and pulsed_drive_model is not None:
                raise NotImplementedError("pulsed field model: impulse_response drives through a heterogeneous medium are not implemented")
            if medium is not None and pulsed_medium_model is None:
                raise NotImplementedError("pulsed field model: heterogeneous media are not implemented (homogeneous media, with or without uniform absorption, only)")
            if directivity:
                raise NotImplementedError("pulsed field model: element directivity is not implemented")
            if slab is not None:
                raise NotImplementedError("pulsed field model: the multi-GPU slab / shard paths are not implemented (whole grid on one GPU only)")
            if "complex" in want:
                raise ValueError("pulsed field model: there is no complex output (the field is a peak over time)")
            if trace_voxels is not None and lazy:
                raise ValueError("pulsed field model: the traces are not part of a lazy result (the Solution does not carry them)")
            cycles, dt, t_end, cfl = pulse
            dt, n_t = pulse_time_axis(spacing_m, n, dt, t_end, cfl)
            want = tuple(want) + ("pmax",)
            response = None
            if pulsed_drive_model is not None:     # (the limits raise here, before anything is retired or uploaded)
                from .sim.field import drive_taps
                response = drive_taps(arr, dt)
        self.retire_results()
        if steering_resident:
            # the resident steering table belongs to the resident element table: another transducer (or the same one with edited
            # elements) is refused BEFORE anything is uploaded -- the context, its steering and its plan stay as they were
            if self._table_of(arr)[3] != self._table_key:
                raise ValueError("steering_resident=True, but the transducer differs from the one the resident steering table was solved for "
                                 "(call beamform(arr, ...) again, or pass delays / apod)")
        else:
            self.bind(arr)      # (compares the element table with the resident one and uploads on a difference)
            self.ctx.set_steering(delays, apod)
        flags = nat.OUT_PMAG
        if "intensity" in want:
            flags |= nat.OUT_INTENSITY
        if "complex" in want:
            flags |= nat.OUT_COMPLEX
        if fp8_correction is False:
            flags |= nat.FIELD_FP16_CORRECTION
        if pulse is not None:
            self.ctx.field_pulse(cycles, dt, n_t)
            self._pulsed = True
            if response is not None and response[1]:
                self.ctx.field_pulse_response(*response)
                self._pulse_response = True
            elif getattr(self, "_pulse_response", False):
                self.ctx.field_pulse_response()       # back to the bare burst
                self._pulse_response = False
            flags |= nat.OUT_PMAX
            if "pii" in want:
                flags |= nat.OUT_PII
        elif getattr(self, "_pulsed", False):
            self.ctx.field_pulse(0.0, 0.0, 0)       # back to continuous wave
            self._pulsed = False
        if directivity:
            self.ctx.set_element_apertures(*arr.element_apertures())
            flags |= nat.FIELD_DIRECTIVITY
        self.ctx.field_absorption(0.0 if medium is not None else absorption)
        self.ctx.field_plan(origin_m, spacing_m, n, freq, c, rho, p0_pa, flags=flags, slab=slab)
        if medium is not None and pulse is not None:  # pulsed model through the medium: kernel 2ph (sampled quadrature, one plane per layer)
            if int(medium.get("planes_per_layer", 1)) > 1:
                raise NotImplementedError("pulsed field model through a medium: one plane per layer only")
            self.ctx.field_pulse_medium(medium.get("sound_speed"), medium.get("attenuation"), medium.get("density"))
        elif medium is not None:  # heterogeneous medium: layered straight-ray kernel
            self.ctx.field_set_medium(medium.get("sound_speed"), medium.get("attenuation"), medium.get("density"),
                                      planes_per_layer=int(medium.get("planes_per_layer", 1)), model=medium.get("model", "auto"))
        self.ctx.field_launch()
        self.result_token += 1
        self._pmax_resident = pulse is not None
        if pulse is not None and "pii" in want:
            self._pii_token = self.result_token
        if lazy and "complex" not in want:
            nx = int(n[0]) if slab is None else int(slab[1])
            self._live_result = DeviceResult(self, self.ctx.n_foci, (nx, int(n[1]), int(n[2])), want)
            return self._live_result
        if "complex" in want:
            outs = [self.ctx.field_fetch(f, want=want) for f in range(self.ctx.n_foci)]
            return {k: np.stack([o[k] for o in outs], axis=0) for k in outs[0]}
        out = self.ctx.field_fetch_all(want=want)
        if trace_voxels is not None:
            out["trace"] = self.ctx.field_pulse_trace(trace_voxels)
        return out

    # ---- kernel 4 -----------------------------------------------------------------------------
    def steering_map(self, arr, origin_m, spacing_m, n, freq, c, p0_pa, apod=(nat.APOD_UNIFORM, 1.0, 0.0), absorption=0.0, directivity=False,
                     medium=None):
        """Focal pressure [Pa] when ``arr`` is steered to each voxel of the grid and the number of contributing elements there ->
        (float32 [nx, ny, nz], int32 [nx, ny, nz]) (olx_steer_map, kernel 4).  ``apod`` = the apodization's kernel-1 arguments,
        ``absorption`` [Np/m] a uniform absorption, ``directivity`` the elements' piston factor.  The volumes are buffers of their own:
        the plan, the steering table and the resident results stay as they are -- unless the element table (or, with ``directivity``,
        the apertures) has to be uploaded, which un-plans the context: arrays handed out lazily are brought to the host first.
        ``medium`` = dict(sound_speed=, attenuation= (volumes or None), comp= None | "equalize" | "matched", spreading=, delays= "straight_ray"
        | "direct") runs the map through the medium along straight rays instead (olx_steer_map_medium, kernel 4h; c = the reference speed,
        ``absorption`` must be 0: the attenuation is the volume's)."""
        if self.ctx.comm_transport():
            raise NotImplementedError("steering map: a context that belongs to a communicator is not supported (one GPU, whole grid)")
        if directivity or self._table_of(arr)[3] != self._table_key:
            self.retire_results()
        self.bind(arr)
        if directivity:
            self.ctx.set_element_apertures(*arr.element_apertures())
        kind, p0, p1 = apod
        if medium is not None:
            if absorption:
                raise ValueError("steering map: a uniform absorption and a medium exclude each other (put the absorption into the attenuation volume)")
            return self.ctx.steer_map_medium(origin_m, spacing_m, n, freq, c, p0_pa=p0_pa, apod_kind=kind, p0=p0, p1=p1,
                                             sound_speed=medium.get("sound_speed"), attenuation=medium.get("attenuation"), comp=medium.get("comp"),
                                             spreading=bool(medium.get("spreading", False)), delays=medium.get("delays", "straight_ray"),
                                             directivity=directivity)
        return self.ctx.steer_map(origin_m, spacing_m, n, freq, c, p0_pa=p0_pa, apod_kind=kind, p0=p0, p1=p1, absorption=absorption,
                                  directivity=directivity)

    # ---- kernel 3 -----------------------------------------------------------------------------
    def thermal(self, origin_m, spacing_m, n, medium, perfusion, schedule, n_foci, dt, baseline, intensity=None, points=None, pii_source=False):
        """Thermal model (sim/thermal.py, kernel 3) -> (rise_max [K], CEM43 [min], traces [n_steps, P] rise [K]), float32.
        ``medium = (density, specific_heat, conductivity, absorption [Np/m])``, each a float or a [nx, ny, nz] volume;
        ``schedule = (row_ptr, focus, tau)``; ``intensity`` [F, nx, ny, nz] W/cm^2 is uploaded once, None reads the resident
        intensity in place, ``pii_source`` the resident pulse intensity integrals.  The field / aggregate volumes and every lazy array over them are left as they are."""
        self.ctx.thermal_plan(origin_m, spacing_m, n, *medium, perfusion=perfusion)
        self.ctx.thermal_schedule(*schedule, points=points)
        if pii_source:      # the resident pulse intensity integrals, read in place (the schedule's on-times carry 1 / pulse length)
            if not self.pii_resident():
                raise RuntimeError("no pulse intensity integrals resident for the current device result")
            self.ctx.thermal_source_pii(n_foci)
        else:
            self.ctx.thermal_source(n_foci, intensity)
        self.ctx.thermal_run(dt, baseline)
        return self.ctx.thermal_fetch()

    # ---- kernel 5 -----------------------------------------------------------------------------
    def fullwave(self, spacing_m, n_padded, medium, c_ref, pml_size, pml_alpha, dt, n_steps, sources, freq, cycles, ramp_cycles=0.0,
                 psq=False, points=None, layer_model="sponge"):
        """Full-wave model (sim/fullwave.py, kernel 5) on the padded grid -> (p_max, p_min, sum p^2 | None, traces [n_steps, P]), float32.
        ``layer_model`` "pml" runs the split layers (olx_fullwave_layers; sources on interior voxels only).
        ``medium = (sound_speed, density, absorption [Np/m])``, each a float or a padded [nx, ny, nz] volume; ``sources = (voxel, amplitude,
        tau)`` per entry, or the element-factored dict of ``_fullwave_sources``; voxels and ``points`` as linear indices of the padded grid.  The field / aggregate / thermal volumes and every lazy
        array over them are left as they are."""
        self.ctx.fullwave_plan(spacing_m, n_padded, *medium, c_ref=c_ref, pml_size=pml_size, pml_alpha=pml_alpha, dt=dt, layer_model=layer_model)
        self._fullwave_sources(sources, spacing_m, medium, dt, freq=freq, cycles=cycles, ramp_cycles=ramp_cycles, n_steps=n_steps, points=points)
        self.ctx.fullwave_run(0, n_steps, psq=psq)
        return self.ctx.fullwave_fetch()

    fullwave_aperture_entries = None     # (element, voxel) entries of the last full-wave source table in element-factored form (None: per-entry form)

    def _fullwave_sources(self, sources, spacing_m, medium, dt, freq, **kw):
        """The source call of a planned full-wave run.  ``sources`` is (voxel, amplitude, tau) per entry -- olx_fullwave_sources -- or a dict,
        the element-factored form of olx_fullwave_sources_elements: {"A" [E], "tau" [E]} plus either "voxels", "elements", "amplitude" per
        entry, or "geometry" = (centre [E, 3] m in the padded grid's frame, u, v, size, n_w, n_l): the rectangles whose weights
        olx_fullwave_apertures forms on the plan, amplitude = W dt c(voxel)^2 4 pi / (2 pi freq h_x h_y h_z).  The dict may carry a drive besides
        the bare burst, applied after the source call: "response" = (class_of_element [E], [taps_c]) -- the drive taps of sim/field.py
        ``drive_taps`` on the plan's dt grid -- or "table" = [n_steps, E] sampled waveforms."""
        if not isinstance(sources, dict):
            self.fullwave_aperture_entries = None
            return self.ctx.fullwave_sources(*sources, freq=freq, **kw)
        if "geometry" in sources:
            row, vox, wt = self.ctx.fullwave_apertures(*sources["geometry"])
            el = np.repeat(np.arange(row.size - 1, dtype=np.int32), np.diff(row))
            c = medium[0]
            c_v = float(c) if np.ndim(c) == 0 else np.asarray(c, dtype=np.float64).reshape(-1)[vox]
            h = np.broadcast_to(np.asarray(spacing_m, dtype=np.float64), (3,))
            amp = wt * float(dt) * c_v ** 2 * 4.0 * np.pi / (2.0 * np.pi * float(freq) * float(np.prod(h)))
        else:
            vox, el, amp = sources["voxels"], sources["elements"], sources["amplitude"]
        self.fullwave_aperture_entries = int(np.size(vox))
        self.ctx.fullwave_sources_elements(vox, el, amp, sources["A"], sources["tau"], freq=freq, **kw)
        if sources.get("response") is not None:      # (class_of_element, [taps_c]): the burst through the drive taps (olx_fullwave_drive_response)
            self.ctx.fullwave_drive_response(*sources["response"])
        if sources.get("table") is not None:         # [n_steps, n_el]: sampled waveforms as they are (olx_fullwave_drive_table)
            self.ctx.fullwave_drive_table(sources["table"])

    def fullwave_steady(self, spacing_m, n_padded, medium, c_ref, pml_size, pml_alpha, dt, n_steps, sources, freq, cycles, ramp_cycles, window,
                        volume=True, receivers=None, layer_model="sponge"):
        """A driven full-wave run with the lock-in at ``freq`` over the steps ``window = (w0, Nw)`` (sim/fullwave.py)
        -> (C, S volumes of the padded grid | None, C_r, S_r float64 [R] | None).  ``receivers = (row, voxel, weight)``: the CSR table, voxels
        linear in the padded grid, or {"geometry": ...} (``_fullwave_sources``): the elements' aperture averages.  The other arguments and what
        is left untouched are ``fullwave``'s."""
        self.ctx.fullwave_plan(spacing_m, n_padded, *medium, c_ref=c_ref, pml_size=pml_size, pml_alpha=pml_alpha, dt=dt, layer_model=layer_model)
        if isinstance(receivers, dict):      # the aperture averages sum_m W_e(m) p(m): the weights' CSR is the receiver table
            receivers = self.ctx.fullwave_apertures(*receivers["geometry"])
        self._fullwave_sources(sources, spacing_m, medium, dt, freq=freq, cycles=cycles, ramp_cycles=ramp_cycles, n_steps=n_steps)
        row, vox, wt = (None, None, None) if receivers is None else receivers
        self.ctx.fullwave_lockin(freq, window[0], window[1], volume=volume, row=row, voxels=vox, weights=wt)
        self.ctx.fullwave_run(0, n_steps)
        return self.ctx.fullwave_fetch_lockin()

    # ---- kernel 6 -----------------------------------------------------------------------------
    def eikonal(self, origin_m, spacing_m, n, sound_speed, source_m, points=None, init_radius=3.0, max_sweeps=None, volume=False):
        """First-arrival travel times from ``source_m`` through ``sound_speed`` (a float, or a [nx, ny, nz] volume) on the grid
        (bf/delay_methods/eikonal.py, kernel 6) -> (T [P] float64 at the ``points = (row, voxel, weight)`` CSR table | None, sweeps,
        T volume float32 | None).  The field / aggregate / thermal / full-wave volumes and every lazy array over them are left as they are."""
        sweeps = self.ctx.eikonal_solve(origin_m, spacing_m, n, sound_speed, source_m, init_radius=init_radius, max_sweeps=max_sweeps)
        at = None if points is None else self.ctx.eikonal_sample(*points)
        return at, sweeps, (self.ctx.eikonal_fetch() if volume else None)

    def upload_result(self, origin_m, spacing_m, n, pmag, intensity=None):
        """Bind host volumes [F,nx,ny,nz] as the resident result (analysis of a detached Solution)."""
        self.retire_results()
        self.ctx.field_upload(origin_m, spacing_m, n, pmag, intensity)
        self.result_token += 1
        self._pmax_resident = False
        self.__dict__.pop("_plan_sig", None)


_grid_memo: dict = {}


def grid_from_coords(coords):
    """(origin_m[3], spacing_m[3], n[3]) from a params.coords mapping; raises ValueError for
    mixed units like the reference (sim/kwave_if.py:104-106)."""
    dims = list(coords.dims) if hasattr(coords, "dims") else list(coords.keys())
    units = [coords[d].attrs["units"] for d in dims]
    if not all(u == units[0] for u in units):
        raise ValueError("All dimensions must have the same units")
    # calc_solution asks four times per call for the same three vectors: remember the last answer per (values, units)
    vecs = [np.asarray(coords[d].data if hasattr(coords[d], "data") else coords[d], dtype=np.float64) for d in dims]
    key = (tuple(dims), units[0], tuple(v.tobytes() for v in vecs))
    hit = _grid_memo.get(key)
    if hit is not None:
        return [list(h) for h in hit]
    out = _grid_from_vectors(dims, vecs, units[0])
    _grid_memo.clear()
    _grid_memo[key] = tuple(tuple(h) for h in out)
    return out


def _grid_from_vectors(dims, vecs, unit):
    scl = getunitconversion(unit, "m")
    origin, spacing, n = [], [], []
    for d, v in zip(dims, vecs):
        origin.append(v[0] * scl)
        spacing.append((np.diff(v)[0] * scl) if len(v) > 1 else scl)  # dx = diff(coord)[0]*scl, kwave_if.py:20
        n.append(len(v))
        if len(v) > 2 and not np.allclose(np.diff(v), np.diff(v)[0], rtol=1e-6, atol=0):
            raise ValueError(f"coordinate {d} is not uniformly spaced")
    return origin, spacing, n
