"""``run_simulation`` -- the drop-in for the reference's k-Wave adapter at the seam
``openlifu.plan.protocol.run_simulation`` (sim/kwave_if.py:80-146, called from
plan/protocol.py:324-336).

Same signature, same output schema (Dataset{p_max [Pa], p_min [Pa], intensity [W/cm^2]} on
``params.coords``), but not a time-domain k-space solve.  Two field models (``field_model``, an extension
like ``directivity``):
  * ``"cw"`` (default): the steady-state monochromatic point-source superposition accumulated by HIP
    kernel 2 (definition: DESIGN.md section 3, oracle/field_oracle.py); ``p_max == p_min == |p|`` and
    ``cycles/dt/t_end/cfl`` are ignored.
  * ``"pulsed"``: the time-domain Rayleigh sum of ``cycles``-cycle tone bursts with the delays truncated
    to whole steps of ``dt``, sampled at k dt up to ``t_end``: peak positive / peak negative pressure
    (HIP kernel 2p; definition DESIGN.md section 2, time axis ``pulse_time_axis``).  Homogeneous media
    by default; ``medium_model="straight_ray"`` opts in to a heterogeneous ``params``: the same model with the straight-ray sums of
    the medium on every (voxel, element) ray, intensity and PII with the voxel's own impedance (HIP kernel 2ph; sampled quadrature,
    one plane per layer, whole grid on one GPU).  ``drive_model="impulse_response"`` opts in to the transducer's and the elements'
    ``impulse_response``: the drive of ``Transducer.calc_output`` -- the burst convolved with both, resampled to ``dt`` -- instead of the bare
    burst (``drive_taps``; kernel 2p's RESP instantiations, homogeneous media only).  Directivity, impulse responses without that opt-in and
    the multi-GPU paths raise NotImplementedError.  Two opt-in outputs of its time axis:
    ``pulse_intensity_integral=True`` adds PII = 1e-4 dt / (rho c) sum_k p(t_k)^2 [J/cm^2] (PII / (cycles / freq) is the pulse-average
    intensity; ``run_thermal_simulation(pulse_energy=...)`` heats with it), ``record_points`` [P, 3] in the units of ``params.coords``
    adds the waveforms p(t_k) at the nearest voxels to the raw dict ("p_trace" [P, n_t], "t" = k dt, "trace_voxels").
``bli_tolerance/upsampling_rate`` are accepted and ignored; ``gpu`` is accepted and ignored -- there is
no CPU path and a missing MI355X raises.
``ref_values_only=True`` simulates the homogeneous reference medium whatever ``params`` holds, as sim/kwave_if.py:49-56 does.
"""
from __future__ import annotations

import logging

import numpy as np

from ..engine import get_engine, grid_from_coords, pulse_time_axis  # noqa: F401 - pulse_time_axis: part of this module's interface
from ..util import dataset as ds

_ATTRS = {"p_max": {"units": "Pa", "long_name": "PPP"}, "p_min": {"units": "Pa", "long_name": "PNP"},
          "intensity": {"units": "W/cm^2", "long_name": "Intensity"},
          "pulse_intensity_integral": {"units": "J/cm^2", "long_name": "Pulse intensity integral"}}


ALPHA_POWER = 0.9      # the reference's kWaveMedium(alpha_power=0.9), sim/kwave_if.py:57
FIELD_MODELS = ("cw", "pulsed")
PULSED_MEDIUM_MODELS = ("straight_ray",)      # how the pulsed model crosses a heterogeneous medium, opt-in (kernel 2ph)
PULSED_DRIVE_MODELS = ("impulse_response",)   # what drives the elements of the pulsed model besides the bare burst, opt-in (kernel 2p, RESP)
PULSE_RESPONSE_MAX_TAPS, PULSE_RESPONSE_MAX_CLASSES = 256, 4      # include/olx.h OLX_PULSE_RESPONSE_MAX_*


def parse_field_model(value) -> str:
    """``field_model`` of run_simulation / ``SimSetup.options["field_model"]``: "cw" (default, also for None / "") or "pulsed"."""
    model = "cw" if value is None or str(value).strip() == "" else str(value).strip().lower()
    if model not in FIELD_MODELS:
        raise ValueError(f"field_model must be one of {FIELD_MODELS}, got {value!r}")
    return model


def parse_pulsed_medium_model(value):
    """``medium_model`` of run_simulation / ``SimSetup.options["pulsed_medium_model"]``: None (default, also for ""), or "straight_ray"."""
    if value is None or str(value).strip() == "":
        return None
    model = str(value).strip().lower()
    if model not in PULSED_MEDIUM_MODELS:
        raise ValueError(f"the pulsed model's medium_model must be None or one of {PULSED_MEDIUM_MODELS}, got {value!r}")
    return model


def parse_pulsed_drive_model(value):
    """``drive_model`` of run_simulation / ``SimSetup.options["pulsed_drive_model"]``: None (default, also for ""), or "impulse_response"."""
    if value is None or str(value).strip() == "":
        return None
    model = str(value).strip().lower()
    if model not in PULSED_DRIVE_MODELS:
        raise ValueError(f"the pulsed model's drive_model must be None or one of {PULSED_DRIVE_MODELS}, got {value!r}")
    return model


def drive_taps(arr, dt, max_classes=PULSE_RESPONSE_MAX_CLASSES, max_taps=PULSE_RESPONSE_MAX_TAPS, what="pulsed field model"):
    """(class_of_element int32 [N], [taps_r fp64]): the drive taps g_e = H_arr * H_el,e of every element on the ``dt`` grid (DESIGN.md
    section 2), the drive of ``Transducer.calc_output`` being sum_m g_e[m] burst((k - m) dt).  H_arr = the array's response resampled to
    ``dt`` ([1] without one); H_el,e = [1] without a response, [h0] for a length-1 response, else the element's resampled to ``dt``.
    Elements whose taps are exactly equal share a class, numbered by first appearance.  A transducer without any response gives no classes
    (the plain kernel runs).  ValueError, naming the model ``what``, for a class longer than ``max_taps`` or more than ``max_classes`` classes:
    the defaults are the pulsed model's (PULSE_RESPONSE_MAX_TAPS, PULSE_RESPONSE_MAX_CLASSES); the full-wave model keeps its table per element
    and passes ``max_classes = n_el``."""
    max_classes, max_taps = int(max_classes), int(max_taps)
    dt = float(dt)
    n = arr.numelements()
    cls = np.zeros(n, dtype=np.int32)
    has_arr = getattr(arr, "impulse_response", None) is not None
    if not has_arr and all(getattr(el, "impulse_response", None) is None for el in arr.elements):
        return cls, []
    h_arr = np.asarray(arr.interp_impulse_response(dt)[0], dtype=np.float64) if has_arr else np.ones(1)
    one = np.ones(1)
    h_of, index, taps = {}, {}, []      # element response (as given) -> H_el on the dt grid; taps -> class
    for e, el in enumerate(arr.elements):
        ir = getattr(el, "impulse_response", None)
        if ir is None:
            h_el = one
        else:
            key = (np.asarray(ir).tobytes(), el.impulse_dt)
            if key not in h_of:
                h_of[key] = np.asarray(ir, dtype=np.float64) if len(ir) == 1 else np.asarray(el.interp_impulse_response(dt)[0], dtype=np.float64)
            h_el = h_of[key]
        g = np.convolve(h_arr, h_el, mode="full")
        key = g.tobytes()
        if key not in index:
            if len(g) > max_taps:
                raise ValueError(f"{what}: element {e}'s impulse response has {len(g)} taps at dt = {dt:g} s, "
                                 f"at most {max_taps} are supported")
            if len(taps) >= max_classes:
                raise ValueError(f"{what}: the elements carry more than {max_classes} different impulse responses "
                                 f"(at most {max_classes} classes of identical drive taps are supported)")
            index[key] = len(taps)
            taps.append(g)
        cls[e] = index[key]
    return cls, taps


def truncate_delays(delays, dt):
    """The reference's whole-step delays (sim/kwave_if.py: zeros(int(delay / dt)) in front of the drive): floor(tau / dt) dt."""
    return np.floor(np.asarray(delays, dtype=np.float64) / float(dt)) * float(dt)


def check_pulsed_supported(arr, directivity=False, drive_model=None):
    """NotImplementedError, naming the reason, for what the pulsed model does not cover on the transducer side.  ``drive_model=
    "impulse_response"`` (the opt-in) lets the impulse responses through."""
    if directivity:
        raise NotImplementedError("pulsed field model: element directivity is not implemented")
    if drive_model is not None:
        return
    if getattr(arr, "impulse_response", None) is not None:
        raise NotImplementedError("pulsed field model: the transducer's impulse_response is not implemented (the drive is the bare tone burst)")
    if any(getattr(el, "impulse_response", None) is not None for el in arr.elements):
        raise NotImplementedError("pulsed field model: element impulse_response is not implemented (the drive is the bare tone burst)")


def _np_per_m(alpha_db_cm_mhz, freq):
    return float(alpha_db_cm_mhz) * (float(freq) * 1e-6) ** ALPHA_POWER * 100.0 / 8.685889638065035      # dB/cm/MHz^y -> Np/m


def _medium(params, freq, ref_values_only=False):
    """(c_ref, rho_ref, volumes | None, absorption [Np/m]).  ``ref_values_only`` (sim/kwave_if.py:49-56): the reference medium --
    the three ``attrs['ref_value']`` -- whatever the volumes hold.  A medium whose sound speed and density equal the reference values
    EVERYWHERE and whose absorption is one constant (the reference's UniformWater / UniformTissue; its example protocol: water with
    0.0022 dB/cm/MHz) is homogeneous: the homogeneous kernels run, every term carrying exp(-a d) when the constant is not zero
    (olx_field_absorption).  Anything else hands the per-voxel sound speed / attenuation / density volumes to the layered
    straight-ray kernels (olx_field_set_medium)."""
    c = float(params["sound_speed"].attrs["ref_value"])
    rho = float(params["density"].attrs["ref_value"])
    if ref_values_only:
        return c, rho, None, _np_per_m(params["attenuation"].attrs["ref_value"], freq)
    vols, const = {}, {}
    for key in ("sound_speed", "density", "attenuation"):
        if key not in params:
            vols[key], const[key] = None, (c if key == "sound_speed" else rho if key == "density" else 0.0)
            continue
        declared = getattr(params[key], "uniform_value", None)
        if declared is not None:                  # constant volume nobody has touched: no 134 MB scan
            vols[key], const[key] = params[key], float(declared)
            continue
        vol = np.asarray(params[key].data)
        lo, hi = (vol.min(), vol.max()) if vol.size else (0.0, 0.0)
        vols[key], const[key] = vol, (float(lo) if lo == hi else None)
    if const["sound_speed"] == c and const["density"] == rho and const["attenuation"] is not None:
        return c, rho, None, _np_per_m(const["attenuation"], freq)
    out = {}
    for key, ref in (("sound_speed", c), ("density", rho), ("attenuation", 0.0)):
        if vols[key] is None or (const[key] is not None and const[key] == ref):
            out[key] = None                      # equals the value the kernels assume anyway
        else:
            out[key] = np.asarray(params[key].data)
    return c, rho, out, 0.0


def simulate_foci(arr, params, delays, apod, freq, amplitude, want=("pmag", "intensity"),
                  steering_resident=False, slab=None, fp8_correction=None, lazy=False, hetero_planes_per_layer=1,
                  hetero_model="auto", directivity=False, ref_values_only=False, pulse=None, trace_voxels=None, pulsed_medium_model=None,
                  pulsed_drive_model=None):
    """Batched core: F foci in one launch -> dict of float32 arrays [F, nx, ny, nz], or with ``lazy`` a
    ``DeviceResult`` whose volumes stay in HBM until read (``lazy_stack`` wraps it in the reference's schema).
    ``pulse = (cycles, dt, t_end, cfl)``: the pulsed model -- "pmag" holds p_min, "pmax" p_max, "pii" in ``want`` adds the pulse intensity
    integral and ``trace_voxels`` (linear voxel indices) the waveforms there under "trace" [F, P, n_t] (not with ``lazy``).
    ``pulsed_medium_model="straight_ray"`` opts the pulsed model in to a heterogeneous ``params`` (kernel 2ph: sampled quadrature, one plane
    per layer); without it such a ``params`` is refused, and a homogeneous one runs kernel 2p either way.
    ``pulsed_drive_model="impulse_response"`` opts in to the impulse responses of ``arr`` (``drive_taps``; homogeneous media only)."""
    pulsed_medium_model = parse_pulsed_medium_model(pulsed_medium_model)
    pulsed_drive_model = parse_pulsed_drive_model(pulsed_drive_model)
    if pulsed_medium_model is not None and pulse is None:
        raise ValueError("pulsed_medium_model needs the pulsed field model (the continuous-wave model picks its medium kernels by itself)")
    if pulsed_drive_model is not None and pulse is None:
        raise ValueError("pulsed_drive_model needs the pulsed field model (the continuous-wave model has no drive waveform)")
    if pulse is not None:
        check_pulsed_supported(arr, directivity, pulsed_drive_model)
    coords = params.coords
    origin, spacing, n = grid_from_coords(coords)
    c, rho, medium, absorption = _medium(params, freq, ref_values_only)
    if pulse is not None and medium is not None and pulsed_drive_model is not None:
        raise NotImplementedError("pulsed field model: impulse_response drives (drive_model) through a heterogeneous medium are not implemented "
                                  "(kernel 2ph has no response)")
    if pulse is not None and medium is not None and pulsed_medium_model is None:
        raise NotImplementedError("pulsed field model: heterogeneous media are not implemented (homogeneous media, with or without uniform absorption, only)")
    if pulse is not None and medium is not None and int(hetero_planes_per_layer) > 1:
        raise NotImplementedError("pulsed field model through a medium: one plane per layer only (hetero_planes_per_layer > 1 is not implemented)")
    if medium is not None and int(hetero_planes_per_layer) > 1:   # opt-in layered-screen quadrature
        medium["planes_per_layer"] = int(hetero_planes_per_layer)
    if medium is not None:   # "auto": marched ray sums (kernel 2m) when the elements lie below the medium, else sampled (2h)
        medium["model"] = hetero_model
    p0 = float(amplitude) * (1.0 if arr.sensitivity is None else float(arr.sensitivity))
    return get_engine().field(arr, delays, apod, origin, spacing, n, float(freq), c, rho, p0, want=want,
                              slab=slab, steering_resident=steering_resident, medium=medium,
                              fp8_correction=fp8_correction, lazy=lazy, directivity=directivity, absorption=absorption, pulse=pulse,
                              trace_voxels=trace_voxels, pulsed_medium_model=pulsed_medium_model, pulsed_drive_model=pulsed_drive_model)


def parse_pii_option(options) -> bool:
    """``SimSetup.options["pulse_intensity_integral"]``: "1" / "true" / "yes" / True turn it on (default off); it needs
    ``options["field_model"] = "pulsed"`` (the continuous-wave model has no time axis)."""
    options = options or {}
    value = options.get("pulse_intensity_integral", False)
    if isinstance(value, str):
        text = value.strip().lower()
        if text not in ("", "0", "1", "false", "true", "no", "yes"):
            raise ValueError(f'options["pulse_intensity_integral"] must be one of "0" / "1" / "false" / "true" / "no" / "yes", got {value!r}')
        on = text in ("1", "true", "yes")
    else:
        on = bool(value)
    if on and parse_field_model(options.get("field_model", "cw")) != "pulsed":
        raise ValueError('options["pulse_intensity_integral"] needs options["field_model"] = "pulsed" '
                         f'(got field_model = {options.get("field_model", "cw")!r}: the continuous-wave model has no time axis)')
    return on


def parse_pulsed_medium_option(options):
    """``SimSetup.options["pulsed_medium_model"]``: None / "" (default) or "straight_ray" -- the pulsed model through a heterogeneous medium
    (kernel 2ph); ValueError for anything else.  It needs ``options["field_model"] = "pulsed"``."""
    options = options or {}
    model = parse_pulsed_medium_model(options.get("pulsed_medium_model"))
    if model is not None and parse_field_model(options.get("field_model", "cw")) != "pulsed":
        raise ValueError('options["pulsed_medium_model"] needs options["field_model"] = "pulsed" '
                         f'(got field_model = {options.get("field_model", "cw")!r}: the continuous-wave model picks its medium kernels by itself)')
    return model


def parse_pulsed_drive_option(options):
    """``SimSetup.options["pulsed_drive_model"]``: None / "" (default) or "impulse_response" -- the pulsed model driven through the
    transducer's and the elements' impulse responses; ValueError for anything else.  It needs ``options["field_model"] = "pulsed"``."""
    options = options or {}
    model = parse_pulsed_drive_model(options.get("pulsed_drive_model"))
    if model is not None and parse_field_model(options.get("field_model", "cw")) != "pulsed":
        raise ValueError('options["pulsed_drive_model"] needs options["field_model"] = "pulsed" '
                         f'(got field_model = {options.get("field_model", "cw")!r}: the continuous-wave model has no drive waveform)')
    return model


def lazy_stack(result, coords, dim="focal_point_index", internal=False):
    """Dataset{p_max, p_min, intensity}[focal_point_index, x, y, z] (plan/protocol.py:341-347) over a DeviceResult:
    three independent LazyDataArrays (p_max and p_min are separate host arrays once read, as callers scale them
    independently, plan/solution.py:333-334).  A pulsed result's p_max is its own volume ("pmax")."""
    from collections import OrderedDict
    dims = (dim,) + tuple(coords.dims if hasattr(coords, "dims") else coords.keys())
    c = OrderedDict([(dim, np.arange(result.shape[0]))])
    c.update(coords)
    out = {}
    for name, key in (("p_max", "pmax" if "pmax" in result.keys else "pmag"), ("p_min", "pmag"), ("intensity", "intensity")):
        out[name] = result.lazy_array(key, lambda fetch, name=name: ds.LazyDataArray(
            result.shape, np.float32, fetch, coords=c, dims=dims, name=name, attrs=_ATTRS[name]))
    if "pii" in result.keys:       # (Protocol.calc_solution with options["pulse_intensity_integral"]: the Solution carries it)
        name = "pulse_intensity_integral"
        out[name] = result.lazy_array("pii", lambda fetch: ds.LazyDataArray(result.shape, np.float32, fetch, coords=c, dims=dims, name=name,
                                                                            attrs=_ATTRS[name]))
    # (internal: the stand-in Dataset whatever the factories hand out -- calc_solution's working copy when xarray is installed)
    return ds.Dataset(out) if internal else ds.make_dataset(out)


def dataset_from_fields(fields, coords, focus=None):
    """Schema of kwave_if.py:131-145.  p_max and p_min are separate, writable arrays (callers scale
    them independently, plan/solution.py:333-334)."""
    dims = list(coords.dims) if hasattr(coords, "dims") else list(coords.keys())
    sel = (lambda a: a) if focus is None else (lambda a: a[focus])
    pm = sel(fields["pmag"])
    px = sel(fields["pmax"]) if "pmax" in fields else pm      # pulsed model: the peak positive pressure is a volume of its own
    out = {"p_max": ds.make_dataarray(px, coords=coords, dims=dims, name="p_max", attrs=_ATTRS["p_max"]),
           "p_min": ds.make_dataarray(pm.copy(), coords=coords, dims=dims, name="p_min", attrs=_ATTRS["p_min"]),
           "intensity": ds.make_dataarray(sel(fields["intensity"]), coords=coords, dims=dims, name="I",
                                          attrs=_ATTRS["intensity"])}
    return ds.make_dataset(out)


def run_simulation(arr, params, delays=None, apod=None, freq: float = 1e6, cycles: float = 20,
                   amplitude: float = 1, dt: float = 0, t_end: float = 0, cfl: float = 0.5,
                   bli_tolerance: float = 0.05, upsampling_rate: int = 5, gpu: bool = True,
                   ref_values_only: bool = False, directivity: bool = False, field_model: str = "cw",
                   pulse_intensity_integral: bool = False, record_points=None, medium_model=None, drive_model=None):
    n = arr.numelements()
    pulse = (float(cycles), float(dt), float(t_end), float(cfl)) if parse_field_model(field_model) == "pulsed" else None
    medium_model = parse_pulsed_medium_model(medium_model)
    if medium_model is not None and pulse is None:
        raise ValueError('medium_model needs field_model="pulsed" (the continuous-wave model picks its medium kernels by itself)')
    drive_model = parse_pulsed_drive_model(drive_model)
    if drive_model is not None and pulse is None:
        raise ValueError('drive_model needs field_model="pulsed" (the continuous-wave model has no drive waveform)')
    if pulse is None and (pulse_intensity_integral or record_points is not None):
        raise ValueError('pulse_intensity_integral and record_points need field_model="pulsed" (the continuous-wave model has no time axis)')
    want, trace_voxels = ("pmag", "intensity"), None
    if pulse_intensity_integral:
        want += ("pii",)
    if record_points is not None:
        from .thermal import _trace_voxels      # (the same nearest-voxel rule as the thermal traces)
        spacing, shape = grid_from_coords(params.coords)[1:]
        trace_voxels, _ = _trace_voxels(record_points, params.coords, shape)
    delays = np.zeros(n) if delays is None else np.asarray(delays, dtype=np.float64)
    apod = np.ones(n) if apod is None else np.asarray(apod, dtype=np.float64)
    if delays.shape != (n,) or apod.shape != (n,):
        raise ValueError(f"delays and apod must have shape ({n},), got {delays.shape} and {apod.shape}")
    logging.info("Running simulation")
    # (directivity: this path's extension -- the far-field pattern of the rectangular elements k-Wave models as finite sources)
    fields = simulate_foci(arr, params, delays[None, :], apod[None, :], freq, amplitude, want=want, directivity=directivity,
                           ref_values_only=ref_values_only, pulse=pulse, trace_voxels=trace_voxels, pulsed_medium_model=medium_model,
                           pulsed_drive_model=drive_model)
    logging.info("Simulation Complete")
    if ref_values_only:
        # The reference then SIMULATES the reference medium (get_medium, sim/kwave_if.py:49-56) but still forms the intensity with
        # the volumes' own impedance, Z = params['density'].data * params['sound_speed'].data (:140-141): the pressure is the uniform
        # run's bit for bit, the intensity follows the volumes where they differ from the reference values.
        z_ref = float(params["density"].attrs["ref_value"]) * float(params["sound_speed"].attrs["ref_value"])
        uniform = all(getattr(params[k], "uniform_value", None) is not None for k in ("density", "sound_speed"))
        Z = None if uniform else np.asarray(params["density"].data, dtype=np.float64) * np.asarray(params["sound_speed"].data, dtype=np.float64)
        if Z is not None and not np.all(Z == z_ref):
            fields = dict(fields)
            fields["intensity"] = (1e-4 * fields["pmag"].astype(np.float64) ** 2 / (2.0 * Z)[None]).astype(np.float32)
    dataset = dataset_from_fields(fields, params.coords, focus=0)
    raw = {"p_max": fields["pmax"][0] if "pmax" in fields else fields["pmag"][0], "p_min": -fields["pmag"][0], "backend": "openlifu_amd/hip-gfx950"}
    if pulse_intensity_integral:
        dims = list(params.coords.dims) if hasattr(params.coords, "dims") else list(params.coords.keys())
        dataset["pulse_intensity_integral"] = ds.make_dataarray(fields["pii"][0], coords=params.coords, dims=dims, name="pulse_intensity_integral",
                                                                attrs=_ATTRS["pulse_intensity_integral"])
        raw["pulse_intensity_integral"] = fields["pii"][0]
    if trace_voxels is not None:
        step = pulse_time_axis(spacing, shape, pulse[1], pulse[2], pulse[3])[0]
        raw["p_trace"], raw["t"], raw["trace_voxels"] = fields["trace"][0], np.arange(fields["trace"].shape[-1]) * step, trace_voxels
    return dataset, raw
