"""Focal-frame helpers and the device-side part of ``Solution.analyze``
(mirror of plan/solution_analysis.py:232-442 as far as ``Solution.scale`` needs it).

Implemented on the device, volumes never leave HBM: the focal ellipsoid masks (``get_mask``) and
masked / global peaks (``field_masked_peak_k``) that give ``mainlobe_pnp_MPa`` -- the only analysis
output ``compute_scaling_factors`` consumes (plan/solution.py:301-303) -- sidelobe and global peaks,
the -3 dB centroid (``field_masked_moments_k``, find_centroid :306-317), beam widths from trilinear
line samples along the focal axes (``field_sample_k``; interp_transformed_axis / get_beam_bounds /
get_beamwidth :444-574) and the time-average intensity peaks (``field_weighted_sum_k``, get_ita).
Emitted pressure / power / TIC (plan/solution.py:152-154, 191-193, 268-276) are a few scalars per focus from the
drive signal; they are host arithmetic on `Transducer.calc_output`, like the reference.
"""
from __future__ import annotations

import json
from dataclasses import dataclass, field
from typing import Dict, Tuple

import numpy as np

from ..util.dict_conversion import DictMixin
from ..util.units import getunittype
from .param_constraint import ParameterConstraint

DEFAULT_ORIGIN = np.zeros(3)


def get_focus_matrix(focus, origin=(0, 0, 0)) -> np.ndarray:
    """Focal frame -> grid coordinates (plan/solution_analysis.py:319-342): z axis along
    origin->focus, x axis in the x-z plane, translation = focus."""
    focus = np.asarray(focus, dtype=float)
    origin = np.asarray(origin, dtype=float)
    zvec = (focus - origin) / np.linalg.norm(focus - origin)
    az = -np.arctan2(zvec[0], zvec[2])
    xvec = np.array([np.cos(az), 0.0, np.sin(az)])
    M = np.eye(4)
    M[:3, 0] = xvec
    M[:3, 1] = np.cross(zvec, xvec)
    M[:3, 2] = zvec
    M[:3, 3] = focus
    return M


def focus_frames(foci, origins) -> np.ndarray:
    """[F, 12] = first three rows of inv(get_focus_matrix(focus_f, origin_f)), row-major, for F foci at once: the same
    arithmetic as ``get_focus_matrix`` per focus (unit vector along origin -> focus, azimuth from atan2, cross product), batched,
    then one batched 4 x 4 inverse."""
    foci = np.atleast_2d(np.asarray(foci, dtype=float)); origins = np.atleast_2d(np.asarray(origins, dtype=float))
    F = foci.shape[0]
    d = foci - origins
    zvec = d / np.sqrt((d * d).sum(axis=1))[:, None]
    az = -np.arctan2(zvec[:, 0], zvec[:, 2])
    xvec = np.stack([np.cos(az), np.zeros(F), np.sin(az)], axis=1)
    M = np.zeros((F, 4, 4))
    M[:, :3, 0] = xvec
    M[:, :3, 1] = np.cross(zvec, xvec)
    M[:, :3, 2] = zvec
    M[:, :3, 3] = foci
    M[:, 3, 3] = 1.0
    return np.linalg.inv(M)[:, :3, :].reshape(F, 12)


@dataclass
class SolutionAnalysisOptions(DictMixin):
    standoff_sound_speed: float = 1500.0
    standoff_density: float = 1000.0
    ref_sound_speed: float = 1500.0
    ref_density: float = 1000.0
    mainlobe_aspect_ratio: Tuple[float, float, float] = (1.0, 1.0, 5.0)
    mainlobe_radius: float = 2.5e-3
    beamwidth_radius: float = 5e-3
    sidelobe_radius: float = 3e-3
    sidelobe_zmin: float = 1e-3
    distance_units: str = "m"
    param_constraints: Dict = field(default_factory=dict)

    def __post_init__(self):
        for label, v in (("Standoff sound speed", self.standoff_sound_speed), ("Standoff density", self.standoff_density),
                         ("Reference sound speed", self.ref_sound_speed), ("Reference density", self.ref_density)):
            if v <= 0:
                raise ValueError(f"{label} must be greater than 0")
        if not isinstance(self.mainlobe_aspect_ratio, (tuple, list)) or len(self.mainlobe_aspect_ratio) != 3:
            raise TypeError("Mainlobe aspect ratio must be a tuple or list of three floats (lat, ele, ax)")
        self.mainlobe_aspect_ratio = tuple(self.mainlobe_aspect_ratio)
        if not all(isinstance(x, (int, float)) for x in self.mainlobe_aspect_ratio):
            raise TypeError("Mainlobe aspect ratio must contain only numbers")
        for label, v, strict in (("Mainlobe radius", self.mainlobe_radius, True), ("Beamwidth radius", self.beamwidth_radius, True),
                                 ("Sidelobe radius", self.sidelobe_radius, True), ("Sidelobe minimum z", self.sidelobe_zmin, False)):
            if not isinstance(v, (int, float)) or (v <= 0 if strict else v < 0):
                raise ValueError(f"{label} must be a {'positive' if strict else 'non-negative'} number")
        if not isinstance(self.distance_units, str):
            raise TypeError("Distance units must be a string")
        if getunittype(self.distance_units) != "distance":
            raise ValueError(f"Distance units must be a length unit, got {self.distance_units}")


@dataclass
class SolutionAnalysis(DictMixin):
    """Per-focus result lists, same field names as the reference (plan/solution_analysis.py:48-112)."""
    mainlobe_pnp_MPa: list = field(default_factory=list)
    mainlobe_isppa_Wcm2: list = field(default_factory=list)
    mainlobe_ispta_mWcm2: list = field(default_factory=list)
    focal_centroid_lat_mm: list = field(default_factory=list)
    focal_centroid_ele_mm: list = field(default_factory=list)
    focal_centroid_ax_mm: list = field(default_factory=list)
    beamwidth_lat_3dB_mm: list = field(default_factory=list)
    beamwidth_ele_3dB_mm: list = field(default_factory=list)
    beamwidth_ax_3dB_mm: list = field(default_factory=list)
    beamwidth_lat_6dB_mm: list = field(default_factory=list)
    beamwidth_ele_6dB_mm: list = field(default_factory=list)
    beamwidth_ax_6dB_mm: list = field(default_factory=list)
    target_position_lat_mm: list = field(default_factory=list)
    target_position_ele_mm: list = field(default_factory=list)
    target_position_ax_mm: list = field(default_factory=list)
    sidelobe_pnp_MPa: list = field(default_factory=list)
    sidelobe_isppa_Wcm2: list = field(default_factory=list)
    sidelobe_to_mainlobe_pressure_ratio: list = field(default_factory=list)
    sidelobe_to_mainlobe_intensity_ratio: list = field(default_factory=list)
    global_pnp_MPa: list = field(default_factory=list)
    global_isppa_Wcm2: list = field(default_factory=list)
    global_ispta_mWcm2: float | None = None
    MI: float | None = None
    TIC: float | None = None
    voltage_V: float | None = None
    p0_MPa: list = field(default_factory=list)
    power_W: float | None = None
    duty_cycle_pulse_train_pct: float | None = None
    duty_cycle_sequence_pct: float | None = None
    sequence_duration_s: float | None = None
    param_constraints: Dict = field(default_factory=dict)

    @classmethod
    def from_dict(cls, parameter_dict):
        d = dict(parameter_dict)
        d["param_constraints"] = {k: v if isinstance(v, ParameterConstraint) else ParameterConstraint.from_dict(v)
                                  for k, v in d.get("param_constraints", {}).items()}
        return cls(**d)

    def to_table(self, constraints=None, focus_index=None):
        """Display table of the reference (plan/solution_analysis.py:146-195, pandas): outside this build's scope -- an explicit refusal instead of
        an AttributeError.  The numbers are the dataclass fields; ``param_constraints[name].get_status(value)`` gives each one's status."""
        raise NotImplementedError("SolutionAnalysis.to_table (pandas display table) is not part of openlifu_amd; read the fields and use "
                                  "param_constraints[name].get_status(value)")

    @staticmethod
    def from_json(json_string: str) -> "SolutionAnalysis":
        return SolutionAnalysis.from_dict(json.loads(json_string))

    def to_json(self, compact: bool = False) -> str:
        d = self.to_dict()
        return json.dumps(d, separators=(",", ":")) if compact else json.dumps(d, indent=4)


@dataclass
class PulseEnergyAnalysis(DictMixin):
    """``Solution.analyze_pulse_energy``: the dose numbers of a burst, read off the pulse intensity integrals PII_f [J/cm^2] of a pulsed
    Solution under the masks of ``SolutionAnalysisOptions`` (DESIGN.md section 2 "pulse energy").  Per-focus lists unless noted."""
    mainlobe_pii_mJcm2: list = field(default_factory=list)      # peak of PII_f inside the mainlobe mask
    sidelobe_pii_mJcm2: list = field(default_factory=list)      # ... outside the sidelobe radius, z > zmin
    global_pii_mJcm2: list = field(default_factory=list)        # ... over z > zmin
    mainlobe_isppa_Wcm2: list = field(default_factory=list)     # pulse-average intensity: mainlobe PII peak / pulse_length_s
    mainlobe_ispta_mWcm2: list = field(default_factory=list)    # peak of I_ta = sum_f n_f PII_f / sequence_period_s under focus f's mainlobe mask
    global_ispta_mWcm2: float | None = None                     # peak of I_ta over z > zmin
    pulses_per_focus: list = field(default_factory=list)        # n_f: pulses of one train aimed at focus f
    pulse_length_s: float | None = None                         # T = cycles / f0
    sequence_period_s: float | None = None                      # P = pulse_train_interval, or pulse_count pulse_interval when that is 0


def beam_bounds_from_samples(offsets: np.ndarray, values: np.ndarray, cutoff: float):
    """get_beam_bounds (plan/solution_analysis.py:488-535) on a sampled line: last offset <= 0 and first
    offset >= 0 whose value is below ``cutoff`` (NaN samples -- outside the grid -- never qualify)."""
    with np.errstate(invalid="ignore"):
        below = values < cutoff
    neg = offsets[(offsets <= 0) & below]
    pos = offsets[(offsets >= 0) & below]
    return (float(neg[-1]) if neg.size else np.nan), (float(pos[0]) if pos.size else np.nan)


# ---- standalone focal-frame grids (plan/solution_analysis.py:344-442), evaluated on the device ----------------
def _grid_axes(da):
    dims = tuple(da.dims)
    return dims, [np.asarray(da.coords[d].data if hasattr(da.coords[d], "data") else da.coords[d], dtype=np.float64) for d in dims]


def get_gridded_transformed_coords(da, matrix: np.ndarray, as_dataset: bool = True, engine=None):
    """Coordinates of ``da``'s grid in the frame whose transform TO ``da``'s frame is ``matrix``
    (plan/solution_analysis.py:344-363): array [..., 3] or a Dataset of ``d_<dim>`` arrays on ``da.coords``."""
    from .. import get_engine
    from ..util.dataset import make_dataarray, make_dataset
    dims, axes = _grid_axes(da)
    if len(dims) != 3:
        raise ValueError("get_gridded_transformed_coords expects a 3-D DataArray")
    A = np.linalg.inv(np.asarray(matrix, dtype=np.float64))[:3]
    coords, _ = (engine or get_engine()).ctx.offset_grid(*axes, A, want=("coords",))
    if not as_dataset:
        return coords
    return make_dataset({f"d_{d}": make_dataarray(coords[..., i], da.coords, dims=dims) for i, d in enumerate(dims)})


def get_offset_grid(da, focus, origin=DEFAULT_ORIGIN, as_dataset: bool = True, engine=None):
    """Grid of ``da`` in focus coordinates (plan/solution_analysis.py:365-382)."""
    return get_gridded_transformed_coords(da, get_focus_matrix(focus, origin=origin), as_dataset=as_dataset, engine=engine)


def calc_dist_from_focus(da, focus, origin=DEFAULT_ORIGIN, aspect_ratio=(1, 1, 1), as_dataarray: bool = True, engine=None):
    """Distance from the focus under the aspect-scaled focal metric (plan/solution_analysis.py:384-403)."""
    from .. import get_engine
    from ..util.dataset import make_dataarray
    dims, axes = _grid_axes(da)
    A = np.linalg.inv(get_focus_matrix(focus, origin=origin))[:3]
    _, dist = (engine or get_engine()).ctx.offset_grid(*axes, A, aspect=np.asarray(aspect_ratio, dtype=np.float64), want=("dist",))
    return make_dataarray(dist, da.coords, dims=dims) if as_dataarray else dist


def get_mask(da, focus, distance: float, origin=DEFAULT_ORIGIN, aspect_ratio=(1, 1, 1), operator: str = "<", engine=None):
    """Boolean mask of the focal ellipsoid (plan/solution_analysis.py:405-442)."""
    from ..util.dataset import make_dataarray
    if operator not in ("<", "<=", ">", ">="):
        raise ValueError("Operator must be '<', '>', '<=', or '>='.")
    dist = calc_dist_from_focus(da, focus, origin=origin, aspect_ratio=aspect_ratio, as_dataarray=False, engine=engine)
    mask = {"<": np.less, "<=": np.less_equal, ">": np.greater, ">=": np.greater_equal}[operator](dist, distance)
    return make_dataarray(mask, da.coords, dims=tuple(da.dims))


# ---- standalone reductions over ONE volume (plan/solution_analysis.py:306-317, 444-574), evaluated on the device ---------------
def _volume_on_device(da, engine=None):
    """Bind the 3-D DataArray ``da`` as the engine's resident one-focus result (``olx_field_upload``; outstanding lazy results are
    brought to the host first) and return (engine, dims, axes in metres, metres per coordinate unit)."""
    from .. import get_engine
    from ..engine import grid_from_coords
    from ..util.units import getunitconversion
    dims, axes = _grid_axes(da)
    if len(dims) != 3:
        raise ValueError("expected a 3-D DataArray (one focus volume)")
    units = [da.coords[d].attrs.get("units", "m") for d in dims]
    coords = {d: da.coords[d] for d in dims}
    for d, u in zip(dims, units):
        if "units" not in coords[d].attrs:
            coords[d].attrs["units"] = u
    origin, spacing, n = grid_from_coords(coords)
    eng = engine or get_engine()
    vol = np.ascontiguousarray(np.asarray(da.data), dtype=np.float32)[None]
    eng.upload_result(origin, spacing, n, vol)
    to_m = getunitconversion(units[0], "m")
    return eng, dims, [a * to_m for a in axes], to_m


def find_centroid(da, cutoff: float, units=None, engine=None) -> np.ndarray:
    """Centroid of the region where ``da > cutoff`` (plan/solution_analysis.py:306-317): sum(da x) / sum(da) over the thresholded
    voxels, per dimension, in the coordinates' own units or converted to ``units``.  The four sums are ``field_masked_moments_k``'s
    (fp64 accumulation on the device over an all-embracing mask)."""
    from ..util.units import getunitconversion
    if units is not None and getunittype(units) != "distance":
        raise ValueError(f"Units must be a length unit, got {units}")
    eng, dims, _, to_m = _volume_on_device(da, engine)
    A = np.zeros((1, 12)); A[0, 0] = A[0, 5] = A[0, 10] = 1.0            # identity frame, radius beyond every voxel: no mask
    mom = eng.ctx.field_masked_moments(A, (1.0, 1.0, 1.0), 1e30, np.array([cutoff], dtype=np.float32))[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        centroid = mom[1:] / mom[0] / to_m                               # metres -> the coordinates' units
    if units is not None:
        da_units = [da.coords[d].attrs.get("units", None) for d in dims]
        centroid = np.array([getunitconversion(cu, units) * c for cu, c in zip(da_units, centroid)])
    return centroid


def interp_transformed_axis(da, focus, dim, origin=DEFAULT_ORIGIN, min_offset=None, max_offset=None, engine=None):
    """``da`` sampled along one axis of the focal coordinate system (plan/solution_analysis.py:444-486): ``2 * da.sizes[dim]`` points
    between ``min_offset`` and ``max_offset`` (default: as far as the grid reaches along that focal axis), trilinear interpolation on the
    device (``field_sample_k``; NaN outside the grid, like ``DataArray.interp``).  Returns a 1-D DataArray over ``offset_d<dim>``."""
    from ..util.dataset import make_dataarray
    eng, dims, axes_m, to_m = _volume_on_device(da, engine)
    matrix = get_focus_matrix(focus, origin=origin)
    a = dims.index(dim)
    if min_offset is None or max_offset is None:
        # extreme focal coordinates of the grid: the offset is affine in (x, y, z), so its extremes sit at the eight corners
        inv = np.linalg.inv(matrix)
        _, axes = _grid_axes(da)
        corners = np.array([[axes[0][i], axes[1][j], axes[2][k], 1.0] for i in (0, -1) for j in (0, -1) for k in (0, -1)])
        d = corners @ inv[a]
        min_offset = float(d.min()) if min_offset is None else min_offset
        max_offset = float(d.max()) if max_offset is None else max_offset
    n = int(da.sizes[dim]) * 2
    interp_dim = np.linspace(min_offset, max_offset, n)
    local = np.zeros((n, 4)); local[:, a] = interp_dim; local[:, 3] = 1.0
    xyz = (matrix @ local.T).T[:, :3]
    vals = eng.ctx.field_sample(0, xyz * to_m, which="pmag")
    name = f"offset_d{dim}"
    return make_dataarray(vals.astype(np.asarray(da.data).dtype if np.asarray(da.data).dtype.kind == "f" else np.float64),
                          {name: interp_dim}, dims=(name,), name=getattr(da, "name", None), attrs=dict(getattr(da, "attrs", {})))


def get_beam_bounds(da, focus, dim, cutoff: float, origin=DEFAULT_ORIGIN, min_offset=None, max_offset=None, engine=None):
    """(negoff, posoff): how far along the negative / positive focal ``dim`` axis ``da`` stays above ``cutoff``
    (plan/solution_analysis.py:488-535); NaN where it never drops below."""
    line = interp_transformed_axis(da, focus=focus, dim=dim, origin=origin, min_offset=min_offset, max_offset=max_offset, engine=engine)
    off = np.asarray(line.coords[f"offset_d{dim}"].data, dtype=np.float64)
    return beam_bounds_from_samples(off, np.asarray(line.data), float(cutoff))


def get_beamwidth(da, focus, dim, cutoff=None, origin=DEFAULT_ORIGIN, min_offset=None, max_offset=None, engine=None) -> float:
    """FWHM (or the width at ``cutoff``) of ``da`` along a focal axis (plan/solution_analysis.py:537-574)."""
    if cutoff is None:
        cutoff = float(np.asarray(da.data).max()) / 2
    negoff, posoff = get_beam_bounds(da, focus=focus, dim=dim, cutoff=float(cutoff), origin=origin, min_offset=min_offset, max_offset=max_offset,
                                     engine=engine)
    return posoff - negoff
