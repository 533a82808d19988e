"""Scenes and drive taps of the impulse-response tests of the pulsed model (kernel 2p's RESP instantiations), shared by
tests/test_gpu_pulsed_response.py (the kernel against the oracle) and tests/test_pulsed_response_host.py (the arrival margins and the
tap conditioning of every case, from the oracle alone).  Every grid origin carries test_gpu_pulsed.py's SHIFT (off the lattice on which
whole families of voxels have t_e / dt exactly on an integer).

Base scene: 13 x 11 x 15 voxels at 0.5 mm from z = 4 mm, 400 kHz, 3 cycles, default dt (1 / 15 of a period) and t_end.  The default
t_end of so small a grid (46 samples) ends inside the burst of most voxels; cases that are about the ring-down say their own t_end.  The
2-tap [1, -1] response runs at dt = 0.25 us (10 samples per period): at the default dt its |H(f0)| = 2 sin(pi / 15) would put
sum |g| / |H(f0)| at 4.8, above the 4 every case keeps so that cancellation between taps does not set the gates."""
from __future__ import annotations

import functools

import numpy as np

from openlifu_amd.sim import field as sf
from oracle import bf_oracle as bo
from conftest import synthetic_array
from test_gpu_pulsed import C, F0, P0, RHO, SHIFT      # noqa: F401 - the common setup, re-exported
import pulsed_response_oracle as pro

DT0 = 0.5 * 0.5e-3 / 1500.0        # the base scene's default dt


def damped_sine(m, dt, periods_decay=1.5, phase=0.3):
    """m taps of exp(-t / tau) sin(2 pi f0 t + phase) sampled at ``dt``: a transducer ringing at the drive frequency."""
    t = np.arange(m) * dt
    return np.exp(-t * F0 / periods_decay) * np.sin(2.0 * np.pi * F0 * t + phase)


def _classes_9x9():
    """9 x 9 array: columns 0-5 ring (class 0), columns 6-7 carry the element scalar [0.5] (class 1), column 8 another response (class 2)
    and is not driven (apod 0)."""
    col = np.arange(81) % 9
    return np.where(col < 6, 0, np.where(col < 8, 1, 2)).astype(np.int32)


BASE = dict(arr=(4, 4, 3.0), n=(13, 11, 15), h=0.5, z0=4.0, foci=[[0, 0, 8.0]], cycles=3, dt=0.0, t_end=0.0, absorption=0.0, cls=None, off=None)
TWO = [[0, 0, 8.0], [1.5, -1.0, 6.0]]
CASES = {
    "ring30":           dict(BASE, foci=TWO, taps=lambda dt: [damped_sine(30, dt)]),
    "ring30_absorbing": dict(BASE, absorption=4.0, taps=lambda dt: [damped_sine(30, dt)]),
    "ring30_whole":     dict(BASE, t_end=2.4e-5, taps=lambda dt: [damped_sine(30, dt)]),
    "classes_9x9":      dict(BASE, arr=(9, 9, 3.0), foci=TWO, t_end=2e-5, cls=_classes_9x9(), off=2,
                             taps=lambda dt: [damped_sine(20, dt), np.array([0.5]), damped_sine(12, dt, 0.8, 1.1)]),
    "two_tap":          dict(BASE, dt=2.5e-7, t_end=2e-5, taps=lambda dt: [np.array([1.0, -1.0])]),
    "longer_than_burst": dict(BASE, t_end=3e-5, taps=lambda dt: [damped_sine(70, dt, 3.0)]),
    "taps255":          dict(BASE, t_end=6e-5, taps=lambda dt: [damped_sine(255, dt, 9.0)]),
    "taps256":          dict(BASE, t_end=6e-5, taps=lambda dt: [damped_sine(256, dt, 9.0, 0.9)]),
    "cut_ringdown":     dict(BASE, foci=TWO, t_end=1.8e-5, taps=lambda dt: [damped_sine(60, dt, 3.0)]),
    "two_pass":         dict(BASE, n=(3, 3, 5), h=1.0, z0=6.0, foci=[[0, 0, 10.0]], cycles=60, dt=1.0 / (40 * F0), t_end=2e-4,
                             taps=lambda dt: [damped_sine(100, dt, 1.5)]),
}
# scenes of single tests (their margins are checked on the host like the cases')
CASES["unit_tap"] = dict(BASE, foci=TWO, t_end=2e-5, taps=lambda dt: [np.array([1.0])])
CASES["delayed_unit_tap"] = dict(BASE, t_end=2e-5, taps=lambda dt: [np.array([0.0, 0.0, 0.0, 1.0])])


class Case:
    """One case, built once: geometry, time axis, Direct steering, classes and taps, and (lazily) the oracle's volumes."""

    def __init__(self, name):
        k = CASES[name]
        self.name = name
        pos_mm, _, size = synthetic_array(*k["arr"])
        self.pos_m = pos_mm * 1e-3
        self.area = size[:, 0] * size[:, 1] * 1e-6
        nx, ny, nz = self.n = k["n"]
        h = k["h"] * 1e-3
        self.xs = (np.arange(nx) - (nx - 1) / 2) * h + SHIFT[0]
        self.ys = (np.arange(ny) - (ny - 1) / 2) * h + SHIFT[1]
        self.zs = k["z0"] * 1e-3 + np.arange(nz) * h + SHIFT[2]
        self.sp = [h, h, h]
        self.dmin = 0.5 * h
        self.cycles, self.absorption = k["cycles"], k["absorption"]
        self.dt, self.n_t = sf.pulse_time_axis(self.sp, self.n, k["dt"], k["t_end"], 0.5)
        self.foci_m = np.atleast_2d(k["foci"]) * 1e-3
        steer = [bo.beamform(self.pos_m, np.zeros_like(self.pos_m), f, C) for f in self.foci_m]
        self.delays, self.apod = np.array([s[0] for s in steer]), np.array([s[1] for s in steer])
        self.cls = np.zeros(len(self.pos_m), dtype=np.int32) if k["cls"] is None else k["cls"]
        if k["off"] is not None:
            self.apod[:, self.cls == k["off"]] = 0.0
        self.taps = [np.asarray(t, dtype=np.float64) for t in k["taps"](self.dt)]
        X, Y, Z = np.meshgrid(self.xs, self.ys, self.zs, indexing="ij")
        self.pts = np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1)

    def conditioning(self):
        """max over the classes of sum |g| / |H(f0)|, H(f0) = sum_m g[m] e^{-j 2 pi f0 dt m}."""
        return max(np.abs(g).sum() / abs((g * np.exp(-2j * np.pi * F0 * self.dt * np.arange(len(g)))).sum()) for g in self.taps)

    def focus_voxels(self):
        """Linear index of the voxel nearest to each focus."""
        idx = [[int(np.argmin(np.abs(ax - f[a]))) for a, ax in enumerate((self.xs, self.ys, self.zs))] for f in self.foci_m]
        return np.array([np.ravel_multi_index(i, self.n) for i in idx])

    def trace_voxels(self, count=18):
        """About 20 voxels: the focus voxels, the grid's first and last voxel and a fixed random draw."""
        rng = np.random.default_rng(len(self.name) + 11)
        vox = np.concatenate([self.focus_voxels(), [0, len(self.pts) - 1], rng.integers(0, len(self.pts), size=count)])
        return np.unique(vox)

    def oracle(self, f):
        """The oracle's dict(p, pmax, pmin, pii, margin) of focus f over the whole grid (cached)."""
        return _oracle(self.name, f)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


def run_device(ctx, name, response=True, taps=None, delays=None, pii=True, trace=None, launches=1):
    """One pulsed plan of case ``name`` on ``ctx`` (a _native.Context) -> (volumes dict of the last launch, traces | None).  ``response=False``
    plans the bare burst; ``taps`` / ``delays`` replace the case's; the context is left continuous-wave and without a response."""
    from openlifu_amd import _native as nat
    k = case(name)
    ctx.set_elements(k.pos_m, np.tile([0.0, 0.0, 1.0], (len(k.pos_m), 1)), k.area)
    ctx.set_steering(k.delays if delays is None else delays, k.apod)
    ctx.field_absorption(k.absorption)
    ctx.field_pulse(k.cycles, k.dt, k.n_t)
    if response:
        ctx.field_pulse_response(k.cls, k.taps if taps is None else taps)
    try:
        ctx.field_plan((k.xs[0], k.ys[0], k.zs[0]), k.sp, k.n, F0, C, RHO, P0,
                       flags=nat.OUT_PMAG | nat.OUT_INTENSITY | nat.OUT_PMAX | (nat.OUT_PII if pii else 0))
        for _ in range(launches):
            ctx.field_launch()
        out = ctx.field_fetch_all(want=("pmag", "intensity", "pmax") + (("pii",) if pii else ()))
        out["variant"] = ctx.field_variant()
        tr = None if trace is None else ctx.field_pulse_trace(trace)
        ctx.sync()
    finally:
        ctx.field_pulse_response()
        ctx.field_pulse(0.0, 0.0, 0)
        ctx.field_absorption(0.0)
    return out, tr


@functools.lru_cache(maxsize=None)
def _oracle(name, f):
    k = case(name)
    return pro.response_volumes(k.pts, k.pos_m, k.area, k.delays[f], k.apod[f], k.cls, k.taps, F0, C, RHO, P0, k.cycles, k.dt, k.n_t, k.dmin,
                                k.absorption)
