"""Steering map: the focal pressure the array delivers when it is steered to each voxel of the simulation grid (DESIGN.md section 2
"Steering map", kernel 4 / olx_steer_map), and what a planner derives from it -- the steering gain relative to a reference point, the
-6 dB envelope, and ``TargetConstraints`` boxes for ``Protocol.target_constraints``."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from ..bf.apod_methods import ApodizationMethod, MediumCompensated, Uniform
from ..engine import get_engine, grid_from_coords
from ..sim.field import ALPHA_POWER, _medium
from ..util import dataset as ds
from .target_constraints import TargetConstraints

_ATTRS = {"focal_pressure": {"units": "Pa", "long_name": "Focal pressure when steered to the voxel"},
          "steering_gain_db": {"units": "dB", "long_name": "Steering gain relative to the reference"},
          "n_active": {"units": "", "long_name": "Elements with a non-zero apodization"},
          "medium_gain_db": {"units": "dB", "long_name": "Focal pressure through the medium relative to water"}}
MEDIUM_MODELS = ("straight_ray",)


def _dims(coords):
    return list(coords.dims) if hasattr(coords, "dims") else list(coords.keys())


def _axis(coords, d):
    return np.asarray(getattr(coords[d], "data", coords[d]), dtype=np.float64)


def nearest_voxel(point, coords):
    """(i, j, k) of the voxel nearest ``point`` (a length-3 position in the coordinates' units, or a ``Point``): the nearest-voxel rule
    of the thermal traces; ValueError outside the grid."""
    dims = _dims(coords)
    if hasattr(point, "get_position"):
        point = point.get_position(units=coords[dims[0]].attrs["units"])
    from ..sim.thermal import _trace_voxels
    shape = [len(_axis(coords, d)) for d in dims]
    _, ijk = _trace_voxels(np.asarray(point, dtype=np.float64).reshape(1, 3), coords, shape)
    return tuple(int(v) for v in ijk[0])


def steering_gain_db(pressure, ref_value):
    """20 log10(P / P_ref), -inf where P = 0."""
    p = np.asarray(pressure, dtype=np.float64)
    if not (np.isfinite(ref_value) and ref_value > 0):
        raise ValueError(f"the reference pressure must be finite and > 0, got {ref_value}")
    out = np.full(p.shape, -np.inf)
    np.log10(p / float(ref_value), out=out, where=p > 0)
    return 20.0 * out


def medium_gain_db(pressure, water_pressure):
    """20 log10(P / P_water): -inf where P = 0, NaN where both are 0."""
    p, w = np.asarray(pressure, dtype=np.float64), np.asarray(water_pressure, dtype=np.float64)
    if p.shape != w.shape:
        raise ValueError(f"the two pressure volumes must have one shape, got {p.shape} and {w.shape}")
    with np.errstate(divide="ignore", invalid="ignore"):
        return 20.0 * np.log10(p / w)


@dataclass
class SteeringMap:
    """``dataset`` on the grid's coords: focal_pressure [Pa], steering_gain_db, n_active (and medium_gain_db for a map through a medium);
    ``reference_index`` = the voxel the gain refers to."""
    dataset: object
    reference_index: tuple

    @staticmethod
    def from_volumes(pressure, n_active, coords, reference=None, water_pressure=None) -> "SteeringMap":
        dims = _dims(coords)
        p = np.asarray(pressure)
        shape = tuple(len(_axis(coords, d)) for d in dims)
        if p.shape != shape or np.asarray(n_active).shape != shape:
            raise ValueError(f"volumes must have the grid shape {shape}, got {p.shape} and {np.asarray(n_active).shape}")
        ref = tuple(int(v) for v in np.unravel_index(int(np.argmax(p)), shape)) if reference is None else nearest_voxel(reference, coords)
        gain = steering_gain_db(p, float(p[ref])).astype(np.float32)
        var = {"focal_pressure": p, "steering_gain_db": gain, "n_active": np.asarray(n_active)}
        if water_pressure is not None:
            var["medium_gain_db"] = medium_gain_db(p, water_pressure).astype(np.float32)
        out = {k: ds.make_dataarray(v, coords=coords, dims=dims, name=k, attrs=_ATTRS[k]) for k, v in var.items()}
        return SteeringMap(dataset=ds.make_dataset(out), reference_index=ref)

    def _gain(self):
        return np.asarray(self.dataset["steering_gain_db"].data)

    def envelope(self, db: float = -6.0) -> np.ndarray:
        """Boolean mask of the voxels whose steering gain is >= ``db``."""
        return self._gain() >= float(db)

    def to_target_constraints(self, db: float = -6.0):
        """One ``TargetConstraints`` per grid dimension: along that axis through the reference voxel, the contiguous run of voxels with
        gain >= ``db`` that holds the reference.  ValueError when the reference voxel itself is below ``db``."""
        mask = self.envelope(db)
        ref = self.reference_index
        if not mask[ref]:
            raise ValueError(f"the reference voxel {ref} has a steering gain of {self._gain()[ref]:.2f} dB, below {db} dB")
        coords = self.dataset.coords
        out = []
        for a, d in enumerate(_dims(coords)):
            idx = list(ref)
            idx[a] = slice(None)
            line = mask[tuple(idx)]
            lo = hi = ref[a]
            while lo > 0 and line[lo - 1]:
                lo -= 1
            while hi < len(line) - 1 and line[hi + 1]:
                hi += 1
            v = _axis(coords, d)
            ends = sorted((float(v[lo]), float(v[hi])))
            out.append(TargetConstraints(dim=d, name=coords[d].attrs.get("long_name", d), units=coords[d].attrs["units"], min=ends[0], max=ends[1]))
        return out


def steering_kernel_args(arr, params, apod_method=None, freq=None, amplitude=1.0):
    """Everything ``calc_steering_map`` hands to the engine, checked: (origin, spacing, n, freq, c, p0_pa, apod kernel args, absorption).
    Raises before anything touches the device."""
    apod_method = Uniform() if apod_method is None else apod_method
    if isinstance(apod_method, MediumCompensated):
        raise NotImplementedError("steering map: MediumCompensated apodization is not implemented (its amplitudes depend on the medium along every ray)")
    if not isinstance(apod_method, ApodizationMethod) or not hasattr(apod_method, "kernel_args"):
        raise NotImplementedError(f"steering map: apodization method {type(apod_method).__name__} has no kernel form")
    freq = getattr(arr, "frequency", None) if freq is None else freq
    if freq is None or not np.isfinite(float(freq)) or float(freq) <= 0:
        raise ValueError(f"steering map: needs a frequency > 0 (freq=, or the transducer's), got {freq!r}")
    freq = float(freq)
    c, _, medium, absorption = _medium(params, freq)
    if medium is not None:
        raise NotImplementedError("steering map: heterogeneous media are not implemented (homogeneous media, with or without uniform absorption, only)")
    origin, spacing, n = grid_from_coords(params.coords)
    p0_pa = float(amplitude) * (1.0 if getattr(arr, "sensitivity", None) is None else float(arr.sensitivity))
    return origin, spacing, n, freq, c, p0_pa, apod_method.kernel_args(), absorption


def steering_medium_args(arr, params, apod_method=None, freq=None, amplitude=1.0, delay_method=None):
    """What ``calc_steering_map(medium_model="straight_ray")`` hands to the engine, checked: (origin, spacing, n, freq, c_ref, p0_pa, base
    apod kernel args, absorption [Np/m], medium), ``medium`` = the dict of ``Engine.steering_map`` when kernel 4h runs (a heterogeneous
    medium, or a ``MediumCompensated`` apodization), None when kernel 4 does (a homogeneous medium with a plain apodization).  Raises
    before anything touches the device."""
    from ..bf.delay_methods import Direct, StraightRay
    apod_method = Uniform() if apod_method is None else apod_method
    if not isinstance(apod_method, ApodizationMethod) or not hasattr(apod_method, "kernel_args"):
        raise NotImplementedError(f"steering map: apodization method {type(apod_method).__name__} has no kernel form")
    delay_method = StraightRay() if delay_method is None else delay_method
    if type(delay_method) not in (StraightRay, Direct):
        raise NotImplementedError(f"steering map: delay method {type(delay_method).__name__} has no kernel form (StraightRay or Direct)")
    freq = getattr(arr, "frequency", None) if freq is None else freq
    if freq is None or not np.isfinite(float(freq)) or float(freq) <= 0:
        raise ValueError(f"steering map: needs a frequency > 0 (freq=, or the transducer's), got {freq!r}")
    freq = float(freq)
    c, _, volumes, absorption = _medium(params, freq)
    origin, spacing, n = grid_from_coords(params.coords)
    p0_pa = float(amplitude) * (1.0 if getattr(arr, "sensitivity", None) is None else float(arr.sensitivity))
    compensated = isinstance(apod_method, MediumCompensated)
    if volumes is None and not compensated:
        return origin, spacing, n, freq, c, p0_pa, apod_method.kernel_args(), absorption, None
    c_ref, sound_speed, _, _, _ = StraightRay.medium(params)
    attenuation, _, _, _ = MediumCompensated.medium(params)
    medium = {"sound_speed": sound_speed, "attenuation": attenuation, "comp": None, "spreading": False,
              "delays": "direct" if type(delay_method) is Direct else "straight_ray"}
    if compensated:
        medium["comp"], medium["spreading"] = apod_method.mode, apod_method.spreading
        f_att = apod_method.frequency
        if f_att is not None and f_att != freq and attenuation is not None:
            # the kernel converts the attenuation at ``freq``: a volume scaled by (f_att / freq)^0.9 is the method's own frequency's a [Np/m]
            medium["attenuation"] = (attenuation.astype(np.float64) * (f_att / freq) ** ALPHA_POWER).astype(np.float32)
    return origin, spacing, n, freq, c_ref, p0_pa, apod_method.kernel_args(), 0.0, medium


def calc_steering_map(arr, params, apod_method=None, freq=None, amplitude=1.0, directivity=False, reference=None, medium_model=None,
                      delay_method=None) -> SteeringMap:
    """Steering map of ``arr`` on ``params.coords`` (array frame): every voxel is a candidate target, its value the focal pressure with
    untruncated Direct delays and ``apod_method`` (default ``Uniform()``).  ``freq`` defaults to ``arr.frequency``; the medium must be
    homogeneous, its uniform attenuation enters as exp(-alpha d).  ``reference`` (a position in the coords' units or a ``Point``; default:
    the volume maximum) is the point the gain refers to.

    ``medium_model="straight_ray"`` takes the map through the medium of ``params`` along straight rays (kernel 4h, DESIGN.md section 2
    "Steering map through a medium"): a heterogeneous ``params`` and a ``MediumCompensated`` apodization (its base is the base apodization,
    its own frequency, else ``freq``, converts the attenuation) are accepted, ``delay_method`` is ``StraightRay()`` (default: every term in
    phase), or ``Direct()`` (the residual phase of an uncorrected array).  A homogeneous medium with a plain apodization still runs kernel 4.
    The dataset then also carries ``medium_gain_db`` = 20 log10(P / P_water), P_water = kernel 4's map with the base apodization and no
    absorption on the same grid."""
    if medium_model is not None:
        if medium_model not in MEDIUM_MODELS:
            raise ValueError(f"steering map: medium_model must be None or one of {MEDIUM_MODELS}, got {medium_model!r}")
        origin, spacing, n, freq, c, p0_pa, apod, absorption, medium = steering_medium_args(arr, params, apod_method, freq, amplitude, delay_method)
        eng = get_engine()
        pf, na = eng.steering_map(arr, origin, spacing, n, freq, c, p0_pa, apod=apod, absorption=absorption, directivity=bool(directivity), medium=medium)
        water = pf
        if medium is not None or absorption:
            water, _ = eng.steering_map(arr, origin, spacing, n, freq, c, p0_pa, apod=apod, absorption=0.0, directivity=bool(directivity))
        return SteeringMap.from_volumes(pf, na, params.coords, reference=reference, water_pressure=water)
    origin, spacing, n, freq, c, p0_pa, apod, absorption = steering_kernel_args(arr, params, apod_method, freq, amplitude)
    pf, na = get_engine().steering_map(arr, origin, spacing, n, freq, c, p0_pa, apod=apod, absorption=absorption, directivity=bool(directivity))
    return SteeringMap.from_volumes(pf, na, params.coords, reference=reference)
