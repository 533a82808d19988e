"""Parity matrix of the non-lattice field kernels -- 2a (field_accum_k), 2b (field_shared_k), 2c (field_mfma_k) -- against the fp64 C oracle.

Every array here is non-lattice on purpose (a spherical bowl, the bowl with one axis made asymmetric, a flat matrix whose pitch is no whole
number of voxels, the jittered array), so the planner has to choose among the > 200 instantiations of these three kernels from the array's
mirror folds, the steering's symmetry, the focus count, nz, flatness and the distance class.  One table (CASES) names for every case the
instantiation it must reach -- the string olx_field_variant reports -- and the full volume is compared with oracle.c_oracle.field_on_grid
at the project's gates (|p| 1e-5, complex 3e-5, intensity 2e-5 of the reference maximum; dmin = half the smallest spacing).

Two tests run without a GPU: the coverage test (the table's expected strings reach every (mt, nt, mx, my) of kernel 2c, every entry of
kernel 2b's dispatch table, the six classes of kernel 2a) and the rule test (the generators fold exactly on the intended axes, are rejected as
lattices, sit in the intended distance class, and the planner's documented rule -- restated in plan_rule below -- predicts each expected string)."""
import functools

import numpy as np
import pytest

from openlifu_amd import _native as nat
from oracle import bf_oracle as bo, c_oracle as co, field_oracle as fo
import plan_query
from conftest import synthetic_array
from test_gpu_field import C, F0, P0, RHO, TOL_I, TOL_P, check, setup_ctx

R_BOWL, PITCH = 40.0, 2.3           # mm: radius of curvature, element pitch (4.6 voxels of 0.5 mm: no lattice kernel applies)
QUARTER_WAVE = 0.25 * C / F0 * 1e3  # mm: below it the planner reports "near"
SWEEP_SEED, SWEEP_DRAWS = 20261, 10


# ---- arrays: name -> (positions [mm], orientations [rad], sizes [mm]); folds about x = 0 / y = 0 as named -----------------------------
ARRAYS = {  # name: (kind, n per side, axes whose mirror fold SURVIVES)
    "bowl8": ("bowl", 8, "xy"), "bowl8_x": ("bowl", 8, "x"), "bowl8_y": ("bowl", 8, "y"), "bowl10": ("bowl", 10, "xy"), "bowl20": ("bowl", 20, "xy"),
    "flat8": ("flat", 8, "xy"), "flat8_x": ("flat", 8, "x"), "flat8_y": ("flat", 8, "y"), "flat8_none": ("flat", 8, ""), "jit8": ("jitter", 8, ""),
}


@functools.lru_cache(maxsize=None)
def array(name):
    kind, n, folds = ARRAYS[name]
    if kind == "jitter":
        out = synthetic_array(n, n, 4.0, jitter=True)
    else:
        a, b = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
        keep = np.ones((n, n), dtype=bool)
        if "x" not in folds: keep &= a < n - 1        # the last row along x dropped: no mirror partner about x = 0 any more
        if "y" not in folds: keep &= b < n - 1
        x = ((a - (n - 1) / 2) * PITCH)[keep]; y = ((b - (n - 1) / 2) * PITCH)[keep]      # (a, n - 1 - a) -> exactly (x, -x)
        z = R_BOWL - np.sqrt(R_BOWL ** 2 - x * x - y * y) if kind == "bowl" else np.zeros_like(x)
        pos = np.stack([x, y, z], axis=1)
        # normal = R[:, 2] = (sin az cos el, -sin el, cos az cos el) -> the centre of curvature (0, 0, R) for the bowl, +z for the flat matrix
        ori = np.stack([np.arctan2(-x, R_BOWL - z), np.arcsin(y / R_BOWL), np.zeros_like(x)], axis=1) if kind == "bowl" else np.zeros_like(pos)
        out = pos, ori, np.full((len(x), 2), 0.9 * PITCH)
    for v in out:
        v.setflags(write=False)
    return out


def mirror_perm(pos, axis, tol=1e-9):
    """Element permutation of the mirror image about coordinate 0 of `axis` (positions in mm), or None."""
    img = pos.copy(); img[:, axis] = -img[:, axis]
    d = np.abs(img[:, None, :] - pos[None, :, :]).max(axis=2)
    perm = d.argmin(axis=1)
    return perm if (d[np.arange(len(pos)), perm] <= tol).all() and len(set(perm)) == len(pos) else None


# ---- grids and foci ------------------------------------------------------------------------------------------------------------------------------
H_ISO, H_ANISO = (0.5, 0.5, 0.5), (0.5, 0.6, 0.4)       # mm; the anisotropic one (noclamp cases) tells hx, hy and hz apart


def grid(case):
    """Coordinate vectors [m]: x, y centred on the array's axis (the folds are about the grid centre); z from 5 mm ("noclamp"), from 0.7 mm above
    the highest element under the grid ("near": closer than a quarter wavelength, farther than a voxel) or from 1 mm below the apex ("clamp")."""
    nx, ny, nz = case["n"]
    cls = case["cls"]
    h = case.get("h", H_ANISO if cls == "noclamp" else H_ISO)
    xs = (np.arange(nx) - (nx - 1) / 2) * h[0]; ys = (np.arange(ny) - (ny - 1) / 2) * h[1]
    pos = array(case["arr"])[0]
    under = (np.abs(pos[:, 0]) <= xs[-1]) & (np.abs(pos[:, 1]) <= ys[-1])
    z0 = {"noclamp": 5.0, "near": pos[under, 2].max() + 0.7, "clamp": -1.0}[cls]
    return xs * 1e-3, ys * 1e-3, (z0 + np.arange(nz) * h[2]) * 1e-3


def distance_class(pos, xs, ys, zs):
    """The planner's rule (olx_field_plan): distance of the nearest element to the grid's bounding box against the smallest spacing and a quarter wavelength."""
    lo = np.array([xs[0], ys[0], zs[0]]) * 1e3; hi = np.array([xs[-1], ys[-1], zs[-1]]) * 1e3
    d = np.sqrt((np.maximum(0.0, np.maximum(lo - pos, pos - hi)) ** 2).sum(axis=1)).min()
    hmin = min(xs[1] - xs[0], ys[1] - ys[0], zs[1] - zs[0]) * 1e3
    return "clamp" if d < hmin else ("near" if d < QUARTER_WAVE else "noclamp")


def foci_of(case):
    """[F, 3] m.  "axis": on the array's axis (steering symmetric about both planes); "xaxis" / "yaxis": on that axis only (the other fold's
    columns collapse); "generic": off both; "wheel": a Wheel of F - 1 spokes around the axis."""
    kind, F = case["foci"]
    k = np.arange(F)
    if kind == "wheel":
        return bo.wheel_targets([0, 0, 30.0], True, F - 1, 4.0) * 1e-3
    if kind == "generic":
        rng = np.random.default_rng(case.get("seed", 7) + 131 * F)
        xy = rng.uniform(0.6, 3.0, (F, 2)) * rng.choice([-1.0, 1.0], (F, 2))
        return np.column_stack([xy, rng.uniform(25.0, 38.0, F)]) * 1e-3
    off = 0.9 + 0.7 * k * (-1.0) ** k
    zero = np.zeros(F)
    return np.column_stack([off if kind == "xaxis" else zero, off if kind == "yaxis" else zero, 25.0 + 1.7 * k]) * 1e-3


# ---- the case table ----------------------------------------------------------------------------------------------------------------------------
OUTPUTS = {"pic": ("pmag", "intensity", "complex"), "pi": ("pmag", "intensity"), "p": ("pmag",), "i": ("intensity",)}
FOLDS = {"": (1, 1), "x": (2, 1), "y": (1, 2), "xy": (2, 2)}
APODS = [("uniform", 1.0, 0.0), ("maxangle", 40.0, 0.0), ("piecewise", 60.0, 20.0)]
SHARED_ENTRIES = ([(1, 1, 1, 1, nf) for nf in (2, 4, 8)] +
                  [(2, 1, 1, 1, nf) for nf in (1, 2, 4, 8)] + [(2, 1, 2, 1, nf) for nf in (1, 2, 4)] +
                  [(1, 2, 1, 1, nf) for nf in (1, 2, 4, 8)] + [(1, 2, 1, 2, nf) for nf in (1, 2, 4)] +
                  [(2, 2, 1, 1, nf) for nf in (1, 2, 4, 8)] + [(2, 2, 2, 1, nf) for nf in (1, 2, 4)] +
                  [(2, 2, 1, 2, nf) for nf in (1, 2, 4)] + [(2, 2, 2, 2, nf) for nf in (1, 2)])        # dispatch_shared's OLX_CASE list (k_accum.hip)


def _flatness(arr):
    return "general" if ARRAYS[arr][0] in ("bowl", "jitter") else "flat"


def _mfma(arr, foci, n, cls, out, nt, apod=0, **kw):
    mx, my = FOLDS[ARRAYS[arr][2]]
    want = f"field_mfma_k<mt{4 if n[2] >= 48 else 1},nt{nt},mx{mx},my{my},{_flatness(arr)},{cls}>"
    return dict(arr=arr, foci=foci, n=n, cls=cls, out=out, apod=APODS[apod], pin=None, want=want, **kw)


def _shared(arr, entry, foci, n, cls, out, pin=None):
    want = "field_shared_k<4,mx%d,my%d,dx%d,dy%d,nf%d," % entry + f"{_flatness(arr)},{cls}>"
    return dict(arr=arr, foci=foci, n=n, cls=cls, out=out, apod=APODS[0], pin=pin, want=want)


def _accum(arr, foci, n, cls, out, pin=None):
    return dict(arr=arr, foci=foci, n=n, cls=cls, out=out, apod=APODS[0], pin=pin, want=f"field_accum_k<4,{_flatness(arr)},{cls}>")


def _build_cases():
    cases = {}
    # kernel 2c, every (mt, nt) under every fold pattern: per pattern both flatness values, all three distance classes, all four output sets,
    # odd and even nx / ny against each fold, nz = 16 (mt1, full runs), 45 (mt1, partial last run), 50 (mt4, one partial run), 64 (mt4, full), 67 (mt4, full + partial run)
    nfoci = {"": {1: 3, 2: 11, 4: 19}, "x": {1: 3, 2: 7, 4: 11}, "y": {1: 3, 2: 7, 4: 11}, "xy": {1: 1, 2: 3, 4: 5}}      # columns = foci x images: <= 8, <= 16, <= 32
    arrays = {"": ("jit8", "flat8_none"), "x": ("bowl8_x", "flat8_x"), "y": ("bowl8_y", "flat8_y"), "xy": ("bowl8", "flat8")}
    shapes = [  # (nt, flat?, class, (nx, ny, nz), outputs)
        (1, 0, "noclamp", (12, 11, 16), "pic"), (2, 1, "near", (13, 10, 45), "pi"), (4, 0, "clamp", (13, 11, 45), "p"),
        (1, 1, "clamp", (13, 11, 50), "i"), (2, 0, "near", (12, 11, 67), "pic"), (4, 1, "noclamp", (13, 10, 64), "pi")]
    for folds in ("", "x", "y", "xy"):
        for q, (nt, flat, cls, n, out) in enumerate(shapes):
            cases[f"2c-{folds or 'none'}-nt{nt}-nz{n[2]}"] = _mfma(arrays[folds][flat], ("generic", nfoci[folds][nt]), n, cls, out, nt, apod=q % 3, seed=q)
    cases["2c-xy-7foci-28col"] = _mfma("bowl8", ("generic", 7), (13, 11, 50), "noclamp", "pic", 4, apod=2)
    cases["2c-xy-xaxis-dy-collapses"] = _mfma("bowl8", ("xaxis", 1), (12, 11, 16), "noclamp", "pic", 1)            # 2 columns for 4 images
    cases["2c-xy-yaxis-3foci"] = _mfma("flat8", ("yaxis", 3), (13, 10, 45), "near", "pi", 1)                       # 6 columns, two store targets each
    cases["2c-none-wheel33-two-tiles"] = _mfma("jit8", ("wheel", 33), (13, 11, 50), "noclamp", "pic", 4, apod=1)    # 32 + 1 columns: ragged second tile
    cases["2c-xy-100el-padded"] = _mfma("bowl10", ("generic", 3), (12, 11, 67), "noclamp", "pic", 2)               # 100 elements: 12 zero-weight slots
    cases["2c-x-56el-padded"] = _mfma("bowl8_x", ("generic", 1), (13, 11, 64), "near", "pi", 1)
    cases["2c-xy-400el-nt4-7chunks"] = _mfma("bowl20", ("generic", 5), (12, 11, 45), "noclamp", "pi", 4, apod=2)    # LDS chunks of 64 elements: 6 + a tail of 16
    cases["2c-xy-400el-nt1-2chunks"] = _mfma("bowl20", ("generic", 1), (13, 10, 64), "noclamp", "pic", 1)          # 256 + 144
    # kernel 2b as the default planner uses it: one symmetric focus = one shared column
    cases["2b-default-xy"] = _shared("bowl8", (2, 2, 1, 1, 1), ("axis", 1), (13, 11, 45), "noclamp", "pic")
    cases["2b-default-x"] = _shared("flat8_x", (2, 1, 1, 1, 1), ("axis", 1), (12, 11, 16), "near", "pi")
    cases["2b-default-y"] = _shared("bowl8_y", (1, 2, 1, 1, 1), ("axis", 1), (13, 10, 50), "clamp", "i")
    cases["2b-default-x-off-y"] = _shared("bowl8_x", (2, 1, 1, 1, 1), ("yaxis", 1), (13, 11, 16), "noclamp", "p")   # x-symmetric steering off the axis
    # kernel 2b's whole dispatch table under the "shared" pin: folds from the array, dx / dy from the steering's symmetry, nf from the focus count
    # (the largest power of two with nf <= F and nf dx dy <= 8; F = 3, 5, 9 leave a ragged last tile)
    for q, e in enumerate(SHARED_ENTRIES):
        mx, my, dx, dy, nf = e
        folds = {(1, 1): "", (2, 1): "x", (1, 2): "y", (2, 2): "xy"}[(mx, my)]
        kind = {(1, 1): "axis", (2, 1): "xaxis", (1, 2): "yaxis", (2, 2): "generic"}[(dx if mx == 2 else 2, dy if my == 2 else 2)]
        nm = dx * dy
        F = {1: 1, 2: (9 if nm == 4 else 3) if q % 2 else 2, 4: 9 if (nm == 2 and q % 2) else 5, 8: 9 if q % 2 else 8}[nf]
        cases["2b-pin-mx%d-my%d-dx%d-dy%d-nf%d" % e] = _shared(arrays[folds][q % 2], e, (kind, F), (12, 11, 9), ("noclamp", "near", "clamp")[q % 3], "pic", pin="shared")
    # kernel 2a: flat / general x noclamp / near / clamp, single focus, nz not a multiple of the 4 voxels a lane owns
    for arr in ("jit8", "flat8"):
        for cls in ("noclamp", "near", "clamp"):
            cases[f"2a-pin-{_flatness(arr)}-{cls}"] = _accum(arr, ("generic", 1), (12, 11, 9), cls, "pic", pin="general")
    cases["2a-default-jittered"] = _accum("jit8", ("generic", 1), (13, 11, 50), "near", "p")
    return cases


CASES = _build_cases()


# ---- the planner's documented rule, restated (CPU check of the table; the GPU tests ask the planner itself) ----------------------------
def plan_rule(case):
    pos, ori, _ = array(case["arr"])
    xs, ys, zs = grid(case)
    foci = foci_of(case)
    F, n = len(foci), len(pos)
    steer = [bo.beamform(pos * 1e-3, ori, f, C, apod=case["apod"]) for f in foci]
    cycles = np.array([s[0] for s in steer]) * F0; w = np.array([s[1] for s in steer])     # (equal areas)
    flat = "flat" if (pos[:, 2] == pos[0, 2]).all() else "general"
    cls = distance_class(pos, xs, ys, zs)
    pin = case["pin"]
    perms = [None if pin == "general" else mirror_perm(pos, a) for a in (0, 1)]
    mx, my = (2 if p is not None else 1 for p in perms)

    def same(f1, p1, f2, p2):
        dph = cycles[f1][p1] - cycles[f2][p2]
        return np.allclose(w[f1][p1], w[f2][p2], rtol=1e-12, atol=0) and (np.abs(dph - np.rint(dph))[w[f1][p1] != 0] <= 1e-9).all()
    ident = np.arange(n)
    dx = 2 if mx == 2 and not all(same(f, ident, f, perms[0]) for f in range(F)) else 1
    dy = 2 if my == 2 and not all(same(f, ident, f, perms[1]) for f in range(F)) else 1
    nf = 1
    while pin != "general" and nf * 2 <= F and nf * 2 * dx * dy <= 8:
        nf *= 2
    if pin != "general" and pin != "shared" and dx * dy * nf >= 2:       # kernel 2c: one column per distinct steering vector, tiles of <= 32 columns
        images = [ident] + ([perms[0]] if mx == 2 else []) + ([perms[1]] if my == 2 else []) + ([perms[1][perms[0]]] if mx * my == 4 else [])
        tiles = [[]]
        for f in range(F):
            for p in images:
                hit = next((col for t in tiles for col in t if col[2] < 4 and same(col[0], col[1], f, p)), None)
                if hit is None:
                    if len(tiles[-1]) >= 32: tiles.append([])
                    tiles[-1].append(hit := [f, p, 0])
                hit[2] += 1
        nt = 1
        while nt * 8 < max(len(t) for t in tiles): nt *= 2
        return f"field_mfma_k<mt{4 if len(zs) >= 48 else 1},nt{nt},mx{mx},my{my},{flat},{cls}>"
    if mx * my * nf == 1:
        return f"field_accum_k<4,{flat},{cls}>"
    return f"field_shared_k<4,mx{mx},my{my},dx{dx},dy{dy},nf{nf},{flat},{cls}>"


def test_case_table_covers_every_instantiation():
    want = [c["want"] for c in CASES.values()]
    for mt in (1, 4):
        for nt in (1, 2, 4):
            for mx, my in FOLDS.values():
                assert any(w.startswith(f"field_mfma_k<mt{mt},nt{nt},mx{mx},my{my},") for w in want), (mt, nt, mx, my)
    for mx, my in FOLDS.values():
        mine = [w for w in want if w.startswith("field_mfma_k") and f",mx{mx},my{my}," in w]
        for tag in ("flat", "general", "noclamp", "near", "clamp"):
            assert any(f",{tag}," in w or w.endswith(f",{tag}>") for w in mine), (mx, my, tag)
    default = [c["want"] for c in CASES.values() if c["pin"] is None]
    for mx, my in ((2, 1), (1, 2), (2, 2)):
        assert any(w.startswith(f"field_shared_k<4,mx{mx},my{my},dx1,dy1,nf1,") for w in default), (mx, my)
    pinned = [c["want"] for c in CASES.values() if c["pin"] == "shared"]
    assert len(SHARED_ENTRIES) == 29 and len(set(SHARED_ENTRIES)) == 29
    for e in SHARED_ENTRIES:
        assert any(w.startswith("field_shared_k<4,mx%d,my%d,dx%d,dy%d,nf%d," % e) for w in pinned), e
    assert {w.split(",")[-2] for w in pinned} == {"flat", "general"} and {w.split(",")[-1] for w in pinned} == {"noclamp>", "near>", "clamp>"}
    for flat in ("flat", "general"):
        for cls in ("noclamp", "near", "clamp"):
            assert f"field_accum_k<4,{flat},{cls}>" in want, (flat, cls)
    assert {c["out"] for c in CASES.values() if c["want"].startswith("field_mfma_k")} == set(OUTPUTS)
    assert {c["n"][2] for c in CASES.values() if c["want"].startswith("field_mfma_k")} >= {16, 45, 50, 64, 67}
    assert {c["n"][:2] for c in CASES.values()} >= {(12, 11), (13, 10), (13, 11)}
    for c in CASES.values():
        assert np.prod(c["n"]) <= 25000 and len(array(c["arr"])[0]) <= 400 and c["foci"][1] <= 33


def test_generators_and_table_follow_the_planning_rule():
    for name, (kind, n, folds) in ARRAYS.items():
        pos = array(name)[0]
        for a, axis in enumerate("xy"):
            assert (mirror_perm(pos, a, tol=1e-9) is not None) == (axis in folds), (name, axis)      # (the library asks 1e-12 m; exact here by construction)
            if axis in folds:
                assert np.array_equal(pos[mirror_perm(pos, a)] * [-1 if a == 0 else 1, -1 if a == 1 else 1, 1], pos), (name, axis)
        assert ((pos[:, 2] == pos[0, 2]).all()) == (kind == "flat"), name
        assert (PITCH / np.array(H_ISO[:2]) % 1 != 0).all() and (PITCH / np.array(H_ANISO[:2]) % 1 != 0).all()      # detect_lattice refuses the pitch
    assert {len(array(a)[0]) for a in ("bowl8", "bowl8_x", "bowl10", "bowl20")} == {64, 56, 100, 400}
    for cid, case in CASES.items():
        xs, ys, zs = grid(case)
        assert distance_class(array(case["arr"])[0], xs, ys, zs) == case["cls"], cid
        assert plan_rule(case) == case["want"], (cid, plan_rule(case))
        pos, ori, size = array(case["arr"])                        # the oracle alone: finite, and a maximum to normalise by
        d, a = bo.beamform(pos * 1e-3, ori, foci_of(case)[-1], C, apod=case["apod"])
        ref = co.field_on_grid(xs, ys, zs, pos * 1e-3, size[:, 0] * size[:, 1] * 1e-6, d, a, F0, C, P0, dmin=0.5 * min(xs[1] - xs[0], ys[1] - ys[0], zs[1] - zs[0]))
        assert np.isfinite(ref).all() and np.abs(ref).max() > 0, cid


def test_every_row_reaches_its_variant_in_the_real_decision():
    """Without a GPU: the real decision (olxplan::decide_variant, through tools/plan_query.cpp) produces for every row the string the GPU tests wait for."""
    for cid, case in CASES.items():
        pos, ori, size = array(case["arr"])
        steer = [bo.beamform(pos * 1e-3, ori, f, C, apod=case["apod"]) for f in foci_of(case)]
        line = plan_query.variant(pos * 1e-3, size[:, 0] * size[:, 1] * 1e-6, np.array([s[0] for s in steer]), np.array([s[1] for s in steer]), *grid(case),
                                  F0, C, RHO, P0, OUTPUTS[case["out"]], pin=case["pin"])
        assert line.split(">")[0] + ">" == case["want"], (cid, line, case["want"])


# ---- GPU: every case against the oracle ------------------------------------------------------------------------------------------------------
def measure(ctx, xs, ys, zs, pos_m, area, delays, ap, outputs, want_variant=None, slab=None, refs=None, label="", extra_flags=0, fragments=(),
            directivity=None, absorption=0.0, tag="MATRIX"):
    """Plan (whole grid or the x-slab), launch, fetch `outputs` of every focus and compare them with the oracle over the full volume at
    test_gpu_field.check's gates.  Returns (variant string, worst error per output, fetched volumes, oracle volumes).  extra_flags: plan flags beside
    the outputs (OLX_FIELD_FP16_CORRECTION, OLX_FIELD_DIRECTIVITY); fragments: pieces the variant string must hold after its prefix; directivity /
    absorption: the oracle's per-term factors (the caller has set them on the context); tag: the first word of the printed line."""
    h = (xs[1] - xs[0], ys[1] - ys[0], zs[1] - zs[0])
    ctx.field_plan((xs[0], ys[0], zs[0]), h, (len(xs), len(ys), len(zs)), F0, C, RHO, P0,
                   flags=extra_flags | sum({"pmag": nat.OUT_PMAG, "intensity": nat.OUT_INTENSITY, "complex": nat.OUT_COMPLEX}[o] for o in outputs), slab=slab)
    name = ctx.field_variant()
    if want_variant:
        assert name.startswith(want_variant), (label, name, want_variant)
    for frag in fragments:
        assert frag in name, (label, frag, name)
    ctx.field_launch()
    sl = slice(None) if slab is None else slice(slab[0], slab[0] + slab[1])
    worst = dict.fromkeys(outputs, 0.0)
    vols, refs_out = [], []
    for f in range(delays.shape[0]):
        out = ctx.field_fetch(f, want=outputs)
        ref = refs[f] if refs is not None else co.field_on_grid(xs, ys, zs, pos_m, area, delays[f], ap[f], F0, C, P0, dmin=0.5 * min(h),
                                                                directivity=directivity, absorption=absorption)
        vols.append(out); refs_out.append(ref)
        ref = ref[sl]
        mx = np.abs(ref).max()
        assert np.isfinite(ref).all() and mx > 0, (label, f)
        iref = fo.intensity_wcm2(np.abs(ref), RHO, C); imx = iref.max()
        for o in outputs:
            assert out[o].shape == ref.shape and out[o].dtype == (np.complex64 if o == "complex" else np.float32), (label, o)
            err = {"pmag": lambda: np.abs(out[o] - np.abs(ref)).max() / mx, "complex": lambda: np.abs(out[o] - ref).max() / mx,
                   "intensity": lambda: np.abs(out[o] - iref).max() / imx}[o]()
            worst[o] = max(worst[o], float(err)) if np.isfinite(err) else np.inf
    figures = outputs if tag == "MATRIX" else ("pmag", "intensity", "complex")      # (the later matrices print every column, "-" where not planned)
    print(f"{tag} {label} | {name.split('>')[0]}> | " + " ".join(f"{o}={worst[o]:.2e}" if o in worst else f"{o}=-" for o in figures))
    for o, tol in (("pmag", TOL_P), ("complex", 3 * TOL_P), ("intensity", TOL_I)):
        assert worst.get(o, 0.0) <= tol, (label, name, o, worst)
    return name, worst, vols, refs_out


def run_case(ctx, case, label, want=True):
    pos, ori, size = array(case["arr"])
    pos_m, area, d, ap = setup_ctx(ctx, pos, ori, size, foci_of(case), apod=case["apod"])
    return measure(ctx, *grid(case), pos_m, area, d, ap, OUTPUTS[case["out"]], want_variant=case["want"] if want else None, label=label)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [k for k, c in CASES.items() if not (c["pin"] == "general")])
def test_matrix_case_matches_oracle(ctx, cid, monkeypatch):
    case = CASES[cid]
    if case["pin"]:
        monkeypatch.setenv("OLX_FIELD_VARIANT", case["pin"])
    else:
        monkeypatch.delenv("OLX_FIELD_VARIANT", raising=False)
    run_case(ctx, case, cid)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [k for k, c in CASES.items() if c["pin"] == "general"])
def test_per_pair_kernel_classes_match_oracle(ctx, cid, monkeypatch):
    """Kernel 2a pinned on arrays the planner would fold: flat / general x noclamp / near / clamp, through test_gpu_field.check itself."""
    case = CASES[cid]
    monkeypatch.setenv("OLX_FIELD_VARIANT", "general")
    pos, ori, size = array(case["arr"])
    pos_m, area, d, ap = setup_ctx(ctx, pos, ori, size, foci_of(case), apod=case["apod"])
    check(ctx, *grid(case), pos_m, area, d, ap, want_variant=case["want"])


@pytest.mark.gpu
def test_x_slabs_keep_the_y_fold_and_tile_the_volume(ctx, monkeypatch):
    """The multi-GPU shard unit on a non-lattice array: an x-slab cannot fold x (its mirror image lies in another slab) but keeps the y fold.
    Three slabs of unequal width, each against the oracle; their concatenation against the whole-volume launch, which folds both axes -- another
    association of the same sums, so equal within the gate, not bit for bit."""
    monkeypatch.delenv("OLX_FIELD_VARIANT", raising=False)
    case = dict(arr="bowl8", foci=("generic", 3), n=(13, 11, 50), cls="noclamp", apod=APODS[2])
    pos, ori, size = array(case["arr"])
    pos_m, area, d, ap = setup_ctx(ctx, pos, ori, size, foci_of(case), apod=case["apod"])
    xs, ys, zs = grid(case)
    outputs = OUTPUTS["pic"]
    _, _, whole, refs = measure(ctx, xs, ys, zs, pos_m, area, d, ap, outputs, want_variant="field_mfma_k<mt4,nt2,mx2,my2,general,noclamp>", label="slabs-whole")
    parts = []
    for b, cnt in ((0, 3), (3, 6), (9, 4)):
        parts.append(measure(ctx, xs, ys, zs, pos_m, area, d, ap, outputs, want_variant="field_mfma_k<mt4,nt1,mx1,my2,general,noclamp>",
                             slab=(b, cnt), refs=refs, label=f"slab-{b}+{cnt}")[2])
    for f in range(3):
        mx = np.abs(refs[f]).max()
        imx = fo.intensity_wcm2(mx, RHO, C)
        for o, tol, scale in (("pmag", TOL_P, mx), ("complex", 3 * TOL_P, mx), ("intensity", TOL_I, imx)):
            joined = np.concatenate([p[f][o] for p in parts], axis=0)
            assert joined.shape == whole[f][o].shape and np.abs(joined - whole[f][o]).max() / scale <= tol, (f, o)


@pytest.mark.gpu
def test_seeded_sweep_over_the_default_planner(ctx, monkeypatch):
    """SWEEP_DRAWS random combinations of the table's axes, no pin, no expected variant: whatever the planner picks must pass the gate."""
    monkeypatch.delenv("OLX_FIELD_VARIANT", raising=False)
    rng = np.random.default_rng(SWEEP_SEED)
    names = sorted(a for a in ARRAYS if a != "bowl20")
    seen = []
    for q in range(SWEEP_DRAWS):
        kind = str(rng.choice(["axis", "xaxis", "yaxis", "generic", "generic", "generic"]))
        case = dict(arr=names[rng.integers(len(names))], foci=(kind, int(rng.choice([1, 2, 3, 5, 7]))), seed=int(rng.integers(1000)),
                    n=(int(rng.choice([12, 13])), int(rng.choice([10, 11])), int(rng.choice([16, 45, 50, 64, 67]))),
                    cls=str(rng.choice(["noclamp", "near", "clamp"])), out=str(rng.choice(sorted(OUTPUTS))),
                    apod=APODS[0] if kind != "generic" else APODS[rng.integers(3)])
        seen.append(run_case(ctx, case, f"sweep-{q} {case}", want=False)[0].split(">")[0])
    assert len(set(seen)) >= 3, seen        # (the draws do spread over the instantiations)
