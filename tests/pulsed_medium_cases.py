"""Geometries and media of the pulsed-through-a-medium tests (kernel 2ph), shared by tests/test_gpu_pulsed_medium.py (the kernel against the
oracle) and tests/test_pulsed_medium_host.py (the arrival margins of every case, from the oracle alone).  Every grid origin carries
test_gpu_pulsed.py's SHIFT (off the lattice on which whole families of voxels have t_e / dt exactly on an integer)."""
from __future__ import annotations

import functools

import numpy as np

from openlifu_amd.sim import field as sf
from oracle import bf_oracle as bo
from conftest import synthetic_array
from test_gpu_pulsed import C, F0, P0, RHO, SHIFT      # noqa: F401 - the common setup, re-exported
import pulsed_medium_oracle as pmo

C_BONE, A_BONE, RHO_BONE = 2800.0, 4.0, 1900.0


def wavy_slab(n, k_lo, k_hi):
    """(sound_speed, attenuation, density) float32 [nx, ny, nz]: bone between two wavy faces, with water holes."""
    nx, ny, nz = n
    i, j, k = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    lo = k_lo + np.rint(1.2 * np.sin(0.9 * i + 0.3) * np.cos(0.7 * j))
    hi = k_hi + np.rint(1.2 * np.cos(0.5 * i) * np.sin(0.8 * j + 0.2))
    bone = (k >= lo) & (k <= hi) & ~((i % 5 == 2) & (j % 4 == 1))
    return (np.where(bone, C_BONE, C).astype(np.float32), np.where(bone, A_BONE, 0.0).astype(np.float32),
            np.where(bone, RHO_BONE, RHO).astype(np.float32))


def _array(nx, ny, pitch, z_mm=0.0, offset_mm=(0.0, 0.0)):
    pos, _, size = synthetic_array(nx, ny, pitch)
    pos = pos + np.array([offset_mm[0], offset_mm[1], z_mm])
    return pos, size


#        array (nx, ny, pitch [, z, offset]), grid n at 1 mm, first z [mm], slab, foci [mm], cycles, dt, t_end
CASES = {
    "slab16":       dict(arr=(4, 4, 3.0), n=(13, 11, 24), z0=3.0, slab=(6, 10), foci=[[0, 0, 20.0]], cycles=3, dt=0.0, t_end=5e-5),
    "slab64_2foci": dict(arr=(8, 8, 3.0), n=(12, 12, 18), z0=4.0, slab=(4, 7), foci=[[0, 0, 15.0], [3.0, -2.0, 12.0]], cycles=4, dt=0.0, t_end=0.0),
    "inside16":     dict(arr=(4, 4, 3.0, 9.3, (0.21, -0.17)), n=(11, 10, 20), z0=0.0, slab=(12, 15), foci=[[1.0, 0, 17.0]], cycles=3, dt=3.1e-7, t_end=0.0),
    "below16":      dict(arr=(4, 4, 3.0, 9.3, (0.21, -0.17)), n=(9, 9, 20), z0=0.0, slab=(3, 6), foci=[[0, 0, 15.0]], cycles=3, dt=3.1e-7, t_end=0.0),
    "n1":           dict(arr=(1, 1, 3.0), n=(6, 5, 12), z0=3.0, slab=(3, 5), foci=[[0, 0, 10.0]], cycles=3, dt=0.0, t_end=3e-5),
    "n65":          dict(arr=(13, 5, 1.5), n=(6, 5, 12), z0=3.0, slab=(3, 5), foci=[[0, 0, 10.0]], cycles=3, dt=0.0, t_end=3e-5),
    "n300":         dict(arr=(20, 15, 1.0), n=(6, 5, 12), z0=3.0, slab=(3, 5), foci=[[0, 0, 10.0]], cycles=3, dt=0.0, t_end=3e-5),
    "two_pass":     dict(arr=(4, 4, 3.0), n=(4, 4, 8), z0=6.0, slab=(2, 4), foci=[[0, 0, 10.0]], cycles=60, dt=1.0 / (40 * F0), t_end=2e-4),
}
# further geometries of single tests (their margins are checked on the host like the cases')
CASES["late16"] = dict(CASES["slab16"], t_end=1.4e-5)
CASES["cw_limit"] = dict(arr=(8, 8, 3.0), n=(16, 16, 16), z0=8.0, slab=(3, 6), foci=[[2.0, 0, 18.0]], cycles=30, dt=1.0 / (16 * F0), t_end=1e-4)


class Case:
    """One case, built once: geometry, time axis, medium, Direct steering, and (lazily) the oracle's ray sums."""

    def __init__(self, name):
        k = CASES[name]
        self.name = name
        pos_mm, size = _array(*k["arr"])
        self.pos_m = pos_mm * 1e-3
        self.area = size[:, 0] * size[:, 1] * 1e-6
        self.n = tuple(k["n"])
        h = 1e-3
        self.spacing = (h, h, h)
        self.origin = (-(self.n[0] - 1) / 2 * h + SHIFT[0], -(self.n[1] - 1) / 2 * h + SHIFT[1], k["z0"] * 1e-3 + SHIFT[2])
        self.cycles = k["cycles"]
        self.dt, self.n_t = sf.pulse_time_axis(self.spacing, self.n, k["dt"], k["t_end"], 0.5)
        self.ss, self.att, self.rho = wavy_slab(self.n, *k["slab"])
        self.foci_m = np.atleast_2d(np.asarray(k["foci"], dtype=np.float64)) * 1e-3
        steer = [bo.beamform(self.pos_m, np.zeros_like(self.pos_m), f, C) for f in self.foci_m]
        self.delays, self.apod = np.array([s[0] for s in steer]), np.array([s[1] for s in steer])
        self._sums = {}

    def sums(self, ss=True, att=True):
        """(A, E) [V, N] of the whole grid with the chosen volumes (False = that volume absent)."""
        key = (bool(ss), bool(att))
        if key not in self._sums:
            self._sums[key] = pmo.ray_sums(self.origin, self.spacing, self.n, self.pos_m, F0, C, self.ss if ss else None, self.att if att else None)
        return self._sums[key]

    def oracle(self, f=0, delays=None, ss=True, att=True):
        """(p_max, p_min, margin) [nx, ny, nz] of focus f (``delays`` [F, N] replace the Direct ones)."""
        A, E = self.sums(ss, att)
        d = self.delays if delays is None else delays
        out = pmo.pulsed_medium(self.origin, self.spacing, self.n, self.pos_m, self.area, d[f], self.apod[f], F0, C, P0, self.cycles, self.dt, self.n_t, A, E)
        return tuple(o.reshape(self.n) for o in out)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)
