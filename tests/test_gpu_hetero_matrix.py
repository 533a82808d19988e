"""Parity matrix of the heterogeneous field kernels -- 2h (field_hetero_k, sampled rays) and 2m (field_hmarch_k, marched ray sums) -- against
their fp64 definitions in oracle/field_oracle.c (co.field_on_grid_hetero with planes_per_layer, co.field_hetero_march).

One table (CASES) names for every case the instantiation it must reach: the prefix olx_field_variant reports after olx_field_set_medium
("field_hmarch_k<nf4,clamp,one-sum>", "field_hetero_k<4,nf2,noclamp,layers>") and, for kernel 2m, the launch sequence it appends after the
launch ("; 2m: inside, lookup0 x1, writer0 x1, lookup x1, writer x5, texel x1").  The full volume of every focus is compared with the oracle at
the project's gates (|p| HET_TOL_P = 1e-5, complex 3e-5, intensity 2e-5 of the reference maximum with the voxel's own rho c; dmin = half the
smallest spacing).

The media are two laterally varying slabs of non-trivial planes (a wavy surface on both faces, water holes, in the three-material form a lossy
soft inclusion) with a gap of trivial planes between them, trivial planes below, and the edge media: a non-trivial plane at k = 0, at k = nz - 1,
every plane non-trivial, a medium that is set but uniform, an absorbing-only medium (c = c0: selects the two-sum form), a lossless aberrator
(kappa = 0), and an array whose outer elements sit exactly half a cell inside the lateral border (the threshold of the INSIDE rule).

Three tests run without a GPU: the coverage test (explicit loops over the template parameters), the rule test (a Python restatement of the host
rules -- plan_rule below -- predicts each expected prefix and sequence from the case's geometry and volumes) and the reference-alone test."""
import functools

import numpy as np
import pytest

from openlifu_amd import _native as nat
from oracle import bf_oracle as bo, c_oracle as co
import plan_query
import test_gpu_field_matrix as fm
from test_gpu_field import C, F0, HET_TOL_P, P0, RHO, TOL_I, TOL_P, setup_ctx

PITCH = fm.PITCH                        # mm
SKULL, SOFT = (2800.0, 6.0, 1900.0), (1560.0, 0.9, 1050.0)      # (c [m/s], alpha [dB/cm/MHz^0.9], rho [kg/m^3]); SOFT is not proportional to SKULL
DENSE = (2000.0, 0.0, 1500.0)           # second material of the lossless aberrator
HALF_H = 2.0 ** -10                     # m: the spacing of the half-cell cases -- dyadic, so that (element - origin) / spacing is exact in fp64
SWEEP_SEED, SWEEP_DRAWS = 20262, 10


# ---- arrays: name -> (positions [mm], orientations [rad], sizes [mm]) ---------------------------------------------------------------------------
RECT = {"one": (1, 1), "m7x9": (7, 9), "m10x13": (10, 13), "m20x20": (20, 20)}      # flat matrices, pitch 2.3 mm (the 20 x 20 one as the issue names it)
COUNTS = {"one": 1, "m7x9": 63, "flat8": 64, "bowl10": 100, "m10x13": 130, "m20x20": 400, "half6x5": 30}


def _mm_for(m):
    """The mm value whose product with 1e-3 (what setup_ctx forms) IS the metre value m."""
    v = m * 1e3
    for cand in (v, np.nextafter(v, np.inf), np.nextafter(v, -np.inf)):
        if cand * 1e-3 == m:
            return cand
    raise AssertionError(m)


@functools.lru_cache(maxsize=None)
def array(name):
    if name in ("flat8", "bowl10"):
        return fm.array(name)
    if name == "half6x5":       # pitch = 2 cells of HALF_H: the outer rows lie at +-5 / +-4 cells, half a cell inside a centred 12 x 10 grid
        a, b = np.meshgrid(np.arange(6), np.arange(5), indexing="ij")
        pos = np.array([[_mm_for((2 * i - 5) * HALF_H), _mm_for((2 * j - 4) * HALF_H), 0.0] for i, j in zip(a.ravel(), b.ravel())])
        out = pos, np.zeros_like(pos), np.full((30, 2), 1.7)
    else:
        n, m = RECT[name]
        a, b = np.meshgrid(np.arange(n), np.arange(m), indexing="ij")
        pos = np.stack([(a.ravel() - (n - 1) / 2) * PITCH, (b.ravel() - (m - 1) / 2) * PITCH, np.zeros(n * m)], axis=1)
        if name == "one":
            pos[0, :2] = 0.4, -0.3
        out = pos, np.zeros_like(pos), np.full((n * m, 2), 0.9 * PITCH)
    for v in out:
        v.setflags(write=False)
    return out


# ---- grids ------------------------------------------------------------------------------------------------------------------------------------------
def nz_of(case):
    return sum(case["lay"])


def grid(case):
    """Coordinate vectors [m].  Lateral: centred on the array's axis; "inside": the outermost element 0.75 cells inside the border; "border": the grid
    spans 0.7 of the array (a single element: 0.3 cells outside the first x row); "half": HALF_H cells, the outermost elements EXACTLY half a cell
    inside.  z: from 5 mm with hz = 0.4 mm ("noclamp") or from 1 mm below the lowest element with hz = 0.5 mm ("clamp")."""
    nx, ny = case["n"]
    pos = array(case["arr"])[0]
    ax, ay = np.abs(pos[:, 0]).max(), np.abs(pos[:, 1]).max()
    cx, cy = (nx - 1) / 2, (ny - 1) / 2
    x_shift = 0.0
    if case["ext"] == "half":
        hx = hy = HALF_H
    elif case["arr"] == "one":
        hx, hy = 1.0e-3, 0.8e-3
        if case["ext"] == "border":
            x_shift = pos[0, 0] * 1e-3 + (cx + 0.3) * hx      # xs[0] = element + 0.3 cells
    elif case["ext"] == "inside":
        hx, hy = ax / (cx - 0.75) * 1e-3, ay / (cy - 0.75) * 1e-3
    else:
        hx, hy = 0.7 * ax / cx * 1e-3, 0.7 * ay / cy * 1e-3
    z0, hz = (5.0e-3, 0.4e-3) if case["cls"] == "noclamp" else ((pos[:, 2].min() - 1.0) * 1e-3, 0.5e-3)
    return (np.arange(nx) - cx) * hx + x_shift, (np.arange(ny) - cy) * hy, z0 + np.arange(nz_of(case)) * hz


# ---- media ------------------------------------------------------------------------------------------------------------------------------------------
FORMS = {"two": True, "three": False, "pin2": False, "absorb": False, "lossless": True, "uniform": False}     # form -> one-sum?


@functools.lru_cache(maxsize=None)
def _medium(n, lay, form, seed, span):
    nx, ny = n
    a0, nA, gap, nB, top = lay
    nz = sum(lay)
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    # the wavy surface of _skull_medium (2 mm sin cos over 40 mm) in cells: one period over `span` of the lateral grid, one plane of amplitude
    s = np.sin(2 * np.pi * i / (span * nx) + 0.3 * seed) * np.cos(2 * np.pi * j / (span * ny))
    up = np.rint((1 + s) / 2).astype(int); up -= up.min()
    dn = np.rint((1 - s) / 2).astype(int); dn -= dn.min()
    k = np.arange(nz)[None, None, :]
    mat = np.zeros((nx, ny, nz), dtype=np.int8)          # 0 water, 1 skull, 2 soft / dense
    for lo, cnt in ((a0, nA), (a0 + nA + gap, nB)):
        b = lo + (dn if cnt >= 3 else 0 * dn); t = lo + cnt - 1 - (up if cnt >= 2 else 0 * up)
        mat[(k >= b[..., None]) & (k <= t[..., None])] = 1
    for _ in range(3):                                  # lateral inclusions: water holes through both slabs, 2 x 3 cells
        p, q = rng.integers(0, nx - 1), rng.integers(0, ny - 2)
        mat[p:p + 2, q:q + 3, :] = 0
    if form in ("three", "lossless"):                   # a third material where the skull was, 3 x 2 cells, twice
        for _ in range(2):
            p, q = rng.integers(0, nx - 2), rng.integers(0, ny - 1)
            blk = mat[p:p + 3, q:q + 2, :]
            blk[blk == 1] = 2
    if form == "uniform":
        mat[:] = 0
    third = DENSE if form == "lossless" else SOFT
    vols = []
    for w, col in zip((C, 0.0, RHO), range(3)):
        v = np.full(mat.shape, w, dtype=np.float32)
        v[mat == 1] = SKULL[col]; v[mat == 2] = third[col]
        vols.append(v)
    if form == "absorb":
        vols[0][:] = C
    if form == "lossless":
        vols[1][:] = 0.0
    for v in vols:
        v.setflags(write=False)
    return tuple(vols)


def medium(case):
    """(c, alpha, rho) float32 volumes [nx, ny, nz]: slab A on planes a0 .. a0 + nA - 1, `gap` trivial planes, slab B, `top` trivial planes."""
    return _medium(case["n"], case["lay"], case["form"], case.get("seed", 3), case.get("span", 0.8))


def nontrivial_planes(cvol, avol):
    """olxmed::scan_planes' rule: a plane with any voxel whose float32 sound speed != c_ref or float32 attenuation != 0."""
    return [k for k in range(cvol.shape[2]) if (np.float32(cvol[:, :, k]).astype(np.float64) != C).any() or (np.float32(avol[:, :, k]) != 0).any()]


# ---- the case table ---------------------------------------------------------------------------------------------------------------------------------
OUTPUTS, APODS = fm.OUTPUTS, fm.APODS
NF_OF = lambda F: 8 if F >= 8 else 4 if F >= 4 else 2 if F >= 2 else 1      # noqa: E731  (configure_variant: the largest power of two <= min(F, 8))


def sequence(ext, one, lay, no_texels=False):
    """The launch sequence "; 2m: ..." that launch_hmarch_nf names, from the DECLARED layout (a0, nA, gap, nB, top)."""
    a0, nA, gap, nB, top = lay
    np_ = nA + nB
    side = "border" if ext == "border" else "inside"
    if np_ == 0:
        return f"; 2m: {side}, lookup0 x1"
    tex = one and top >= 16 and not no_texels
    n = {"lookup0": 1 if a0 > 0 else 0, "writer0": 1, "lookup": (1 if gap > 0 and nA > 0 and nB > 0 else 0) + (1 if top > 0 and not tex else 0), "writer": np_ - 1,
         "texel": 1 if tex else 0}
    return f"; 2m: {side}" + "".join(f", {kind} x{cnt}" for kind, cnt in n.items() if cnt)


def _m(arr, F, n, lay, cls, ext, form, out, apod=0, rho=True, core=False, **kw):
    one = FORMS[form]
    want = f"field_hmarch_k<nf{NF_OF(F)},{cls}{',one-sum' if one else ''}>"
    return dict(arr=arr, foci=("generic", F), n=n, lay=lay, cls=cls, ext=ext, form=form, out=out, apod=APODS[apod], rho=rho, core=core, model="auto", G=1,
                want=want, seq=sequence(ext, one, lay), **kw)


def _h(arr, F, n, lay, cls, G, out, apod=0, rho=True, form="two", ext="inside", **kw):
    want = f"field_hetero_k<4,nf{NF_OF(F)},{cls}{',layers' if G > 1 else ''}>"
    return dict(arr=arr, foci=("generic", F), n=n, lay=lay, cls=cls, ext=ext, form=form, out=out, apod=APODS[apod], rho=rho, core=True, model="sampled", G=G,
                want=want, seq=None, **kw)


F_FOR = {1: (1, 1), 2: (2, 3), 4: (5, 4), 8: (11, 8)}       # nf -> focus counts (first: a ragged last tile where there is one: 3 = 2 + 1, 5 = 4 + 1, 11 = 8 + 3)


def _build_cases():
    cases = {}
    outs = ("pic", "pi", "p", "i")
    # kernel 2m, the core: (nf) x (one-sum | two-sum by three materials) x (inside | border) x (clamp | noclamp), 32 cases.  Within each form the eight
    # cases of nf <= 2 and the eight of nf >= 4 go round the six element counts; the one-sum cases alternate a top run of 16 planes (texel look-ups)
    # and of 15 (plain); lookup0 runs of 3 .. 9 planes, gaps of 2 and 3 planes: every residue mod 4 (a look-up block takes 4 planes)
    arrs = {"two": ("m20x20", "one", "m10x13", "m7x9", "bowl10", "flat8", "one", "m10x13"),
            "three": ("bowl10", "flat8", "m7x9", "m20x20", "m10x13", "one", "bowl10", "m7x9")}
    grids = ((12, 10), (13, 16), (18, 21), (25, 16), (12, 33), (13, 21), (18, 10), (25, 21))
    q = 0
    for form in ("two", "three"):
        for ni, nf in enumerate((1, 2, 4, 8)):
            for ei, ext in enumerate(("inside", "border")):
                for ci, cls in enumerate(("noclamp", "clamp")):
                    arr = arrs[form][(ni % 2) * 4 + ei * 2 + ci]
                    a0 = (9 if arr == "bowl10" else 3 + q % 4) if cls == "clamp" else 4 + (q + ni) % 4         # (clamp: the first plane above the bowl's rim, 2.8 mm)
                    top = (16 if (q + ni) % 2 else 15) if form == "two" else (1, 2, 5, 6)[(q + ni) % 4]
                    lay = (a0, 3, 2 + q % 2, 3 if q % 3 else 2, top)
                    F = F_FOR[nf][q % 2]
                    cases[f"2m-nf{nf}-{'one' if form == 'two' else 'two'}-{ext}-{cls}"] = _m(arr, F, grids[(q + ei) % 8], lay, cls, ext, form, outs[(q + q // 4) % 4], apod=q % 3, rho=(q // 2 + q // 8) % 2 == 0,
                                                                                          core=True, seed=q)
                    q += 1
    # the one-sum twins: the same (nf, inside / border, clamp / noclamp) with the other side of the texel threshold (top run 15 <-> 16 planes)
    for cid, c in list(cases.items()):
        if c["form"] != "two":
            continue
        a0, nA, gap, nB, top = c["lay"]
        cases[cid + "-twin"] = _m(c["arr"], c["foci"][1], c["n"], (a0, nA, gap, nB, 31 - top), c["cls"], c["ext"], "two", c["out"], apod=APODS.index(c["apod"]), rho=c["rho"], seed=c["seed"])
    # the pinned two-sum form on the two-material medium (OLX_MARCH_SUMS=2), and element counts the core leaves out per form and focus class
    cases["2m-pin2-nf1-400el"] = _m("m20x20", 1, (12, 16), (5, 3, 3, 3, 6), "noclamp", "inside", "pin2", "pic", pin=True)       # two-sum writers: 25 elements per wave
    cases["2m-pin2-nf4-130el-border-clamp"] = _m("m10x13", 5, (13, 21), (4, 3, 2, 2, 17), "clamp", "border", "pin2", "pi", apod=1, pin=True)
    cases["2m-pin2-nf8-63el"] = _m("m7x9", 8, (18, 10), (6, 2, 3, 3, 3), "noclamp", "border", "pin2", "i", apod=2, rho=False, pin=True)
    cases["2m-two-nf2-130el"] = _m("m10x13", 3, (13, 16), (7, 3, 3, 3, 2), "noclamp", "inside", "three", "pic", apod=1)
    cases["2m-two-nf1-100el"] = _m("bowl10", 1, (12, 21), (6, 3, 2, 3, 3), "noclamp", "border", "three", "pi")
    cases["2m-two-nf2-64el"] = _m("flat8", 2, (13, 10), (5, 3, 3, 2, 4), "clamp", "inside", "three", "p", apod=2)
    cases["2m-two-nf4-400el"] = _m("m20x20", 4, (12, 16), (4, 3, 2, 3, 7), "noclamp", "border", "three", "pi", apod=1)
    cases["2m-two-nf8-64el"] = _m("flat8", 11, (13, 10), (6, 3, 3, 3, 1), "noclamp", "inside", "three", "pic")
    cases["2m-one-nf2-400el"] = _m("m20x20", 3, (12, 16), (6, 3, 2, 3, 19), "clamp", "border", "two", "pi", apod=2)              # one-sum writers: 64 + 36 elements per wave
    cases["2m-one-nf2-100el"] = _m("bowl10", 2, (13, 16), (5, 3, 3, 3, 15), "noclamp", "inside", "two", "pic", apod=1)
    cases["2m-one-nf1-64el"] = _m("flat8", 1, (12, 21), (7, 3, 2, 3, 16), "noclamp", "border", "two", "i", rho=False)
    cases["2m-one-nf1-63el"] = _m("m7x9", 1, (13, 10), (4, 3, 3, 3, 18), "clamp", "inside", "two", "pic", apod=2)
    cases["2m-one-nf4-400el"] = _m("m20x20", 5, (12, 10), (5, 3, 2, 3, 17), "noclamp", "inside", "two", "pi", apod=1)            # look-up chunks of 64: six + a tail of 16
    cases["2m-one-nf8-63el"] = _m("m7x9", 11, (13, 16), (6, 3, 3, 3, 5), "noclamp", "border", "two", "pic")
    cases["2m-one-nf8-64el"] = _m("flat8", 8, (18, 10), (4, 3, 2, 3, 16), "clamp", "inside", "two", "p", apod=2)
    # medium edges
    cases["2m-edge-plane-at-k0"] = _m("flat8", 3, (13, 16), (0, 3, 3, 3, 5), "noclamp", "inside", "two", "pic")
    cases["2m-edge-plane-at-top"] = _m("m7x9", 5, (12, 10), (5, 3, 2, 3, 0), "noclamp", "border", "two", "pi", apod=1)
    cases["2m-edge-every-plane"] = _m("flat8", 2, (13, 10), (0, 4, 0, 3, 0), "noclamp", "inside", "three", "pic")
    cases["2m-edge-every-plane-one-sum"] = _m("m10x13", 1, (12, 16), (0, 5, 0, 4, 0), "noclamp", "inside", "two", "pi", apod=2)
    cases["2m-edge-uniform-medium"] = _m("flat8", 3, (13, 10), (9, 0, 0, 0, 0), "clamp", "inside", "uniform", "pic")
    cases["2m-edge-absorbing-only"] = _m("m7x9", 2, (12, 16), (5, 3, 3, 3, 17), "noclamp", "inside", "absorb", "pic", apod=1)
    cases["2m-edge-lossless-aberrator"] = _m("flat8", 5, (13, 16), (4, 3, 2, 3, 16), "clamp", "border", "lossless", "pic")
    cases["2m-edge-half-cell-inside"] = _m("half6x5", 3, (12, 10), (6, 3, 3, 3, 16), "noclamp", "half", "two", "pic", apod=2)
    cases["2m-edge-half-cell-two-sum-clamp"] = _m("half6x5", 4, (12, 10), (5, 3, 2, 3, 3), "clamp", "half", "three", "pi")
    # kernel 2h: (nf) x (clamp | noclamp) x (no layers | G = 3 | G = 8), slabs of 5 + 4 planes (G = 3: layers of 3 + 2 and 3 + 1 planes)
    q = 0
    for ni, nf in enumerate((1, 2, 4, 8)):
        for ci, cls in enumerate(("noclamp", "clamp")):
            for G in (1, 3 if (ni + ci) % 2 == 0 else 8):
                r = q + q // 4                          # (so that array, grid, outputs and class do not go round together)
                arr = ("flat8", "m7x9", "bowl10", "one")[r % 4]
                a0 = (9 if arr == "bowl10" else 3 + q % 3) if cls == "clamp" else 4 + q % 3
                cases[f"2h-nf{nf}-{cls}-{'G%d' % G if G > 1 else 'planes'}"] = _h(arr, F_FOR[nf][q % 2], ((12, 10), (13, 16), (18, 10), (13, 21))[(r + 1) % 4], (a0, 5, 2 + q % 2, 4, 2 + q % 5), cls, G,
                                                                                    outs[(r + 2) % 4], apod=q % 3, rho=(q // 2 + ni) % 2 == 1, form=("two", "three")[(q // 4) % 2], ext=("inside", "border")[r % 2], seed=q)
                q += 1
    return cases


CASES = _build_cases()
CASES_2M = [k for k, c in CASES.items() if c["model"] == "auto"]
CASES_2H = [k for k, c in CASES.items() if c["model"] == "sampled"]


# ---- the host rules, restated (CPU check of the table; the GPU tests ask the library itself) ---------------------------------------------------------
def plan_rule(case, no_texels=False):
    """(variant prefix, launch sequence or None) from the case's geometry and volumes: olx_field_plan's clamp class, configure_variant's nf,
    olx_field_set_medium's non-trivial planes, march_ok and one-sum test, launch_hmarch_nf's INSIDE rule, texel rule and segment walk."""
    pos_m = array(case["arr"])[0] * 1e-3            # (what setup_ctx hands to olx_set_elements)
    xs, ys, zs = grid(case)
    origin, h = (xs[0], ys[0], zs[0]), (xs[1] - xs[0], ys[1] - ys[0], zs[1] - zs[0])        # (what field_plan receives)
    nx, ny, nz = len(xs), len(ys), len(zs)
    cvol, avol, _ = medium(case)
    nf = NF_OF(case["foci"][1])
    cls = "clamp" if fm.distance_class(array(case["arr"])[0], xs, ys, zs) == "clamp" else "noclamp"      # (olx_field_plan: an element closer to the grid's box than the smallest spacing)
    planes = nontrivial_planes(cvol, avol)
    G = case["G"]
    march_ok = G == 1 and nx >= 2 and ny >= 2 and (not planes or all(ez < origin[2] + planes[0] * h[2] for ez in pos_m[:, 2]))
    if case["model"] == "sampled" or not march_ok:
        return f"field_hetero_k<4,nf{nf},{cls}{',layers' if G > 1 and planes else ''}>", None
    # one-sum form: the float32 stencil values {sig, a'} of every voxel of the non-trivial planes lie on one line through the origin (products in fp64)
    one = False
    if planes:
        lam = C / F0
        afac = (F0 * 1e-6) ** 0.9 * 100.0 * (1.0 / 8.685889638065035) * lam
        sg = np.float32(C / cvol[:, :, planes].astype(np.float64) - 1.0).astype(np.float64).transpose(2, 0, 1).ravel()
        ab = np.float32(avol[:, :, planes].astype(np.float64) * afac).astype(np.float64).transpose(2, 0, 1).ravel()
        nzr = np.flatnonzero((sg != 0) | (ab != 0))
        s_ref, a_ref = sg[nzr[0]], ab[nzr[0]]
        one = s_ref != 0 and bool((sg[nzr] * a_ref == ab[nzr] * s_ref).all()) and not case.get("pin")
    eu, ev = (pos_m[:, 0] - origin[0]) / h[0], (pos_m[:, 1] - origin[1]) / h[1]
    inside = bool(((eu >= 0.5) & (eu <= nx - 1.5) & (ev >= 0.5) & (ev <= ny - 1.5)).all())
    side = "inside" if inside else "border"
    prefix = f"field_hmarch_k<nf{nf},{cls}{',one-sum' if one else ''}>"
    if not planes:
        return prefix, f"; 2m: {side}, lookup0 x1"
    n = dict.fromkeys(("lookup0", "writer0", "lookup", "writer", "texel"), 0)

    def go(k_lo, k_hi, kind):
        if k_hi >= k_lo:
            n[kind] += 1
    go(0, planes[0] - 1, "lookup0"); go(planes[0], planes[0], "writer0")
    for p in range(1, len(planes)):
        go(planes[p - 1] + 1, planes[p] - 1, "lookup"); go(planes[p], planes[p], "writer")
    top_lo = planes[-1] + 1
    go(top_lo, nz - 1, "texel" if one and nz - top_lo >= 16 and not no_texels else "lookup")
    return prefix, f"; 2m: {side}" + "".join(f", {kind} x{cnt}" for kind, cnt in n.items() if cnt)


def test_case_table_covers_every_instantiation():
    core = {k: c for k, c in CASES.items() if c["core"] and c["model"] == "auto"}
    assert len(core) == 32
    for nf in (1, 2, 4, 8):
        for one in (True, False):
            for side in ("inside", "border"):
                for cls in ("clamp", "noclamp"):
                    hit = [k for k, c in core.items() if c["want"] == f"field_hmarch_k<nf{nf},{cls}{',one-sum' if one else ''}>" and c["seq"].startswith(f"; 2m: {side},")]
                    assert len(hit) == 1, (nf, one, side, cls, hit)           # (exactly one: removing any core case fails here)
                    if one:                                                   # the one-sum form with the texel launch and in a twin without it
                        for tex in (True, False):
                            assert any(c["want"] == core[hit[0]]["want"] and c["seq"].startswith(f"; 2m: {side},") and ("texel x1" in c["seq"]) == tex
                                       for c in CASES.values()), (nf, side, cls, tex)
    tops = {c["lay"][4] for c in CASES.values() if "one-sum" in c["want"]}
    assert {15, 16} <= tops                                                   # the texel threshold from both sides
    m2 = [c for c in CASES.values() if c["model"] == "auto"]
    for cnt in (1, 63, 64, 100, 130, 400):                                    # every element count under nf <= 2 and nf >= 4, one-sum and two-sum
        for small in (True, False):
            for one in (True, False):
                assert any(COUNTS[c["arr"]] == cnt and (NF_OF(c["foci"][1]) <= 2) == small and ("one-sum" in c["want"]) == one for c in m2), (cnt, small, one)
    assert {c["form"] for c in m2} == set(FORMS)
    assert any(c["ext"] == "half" and "one-sum" in c["want"] for c in m2) and any(c["ext"] == "half" and "one-sum" not in c["want"] for c in m2)
    runs = {"lookup0": set(), "lookup": set(), "texel": set()}                 # look-up runs of every length mod 4 (a look-up block takes four planes)
    for c in m2:
        a0, nA, gap, nB, top = c["lay"]
        runs["lookup0"].add(a0 % 4); runs["lookup"].add(gap % 4); runs["texel" if "texel" in c["seq"] else "lookup"].add(top % 4)
    assert all(r == {0, 1, 2, 3} for r in runs.values()), runs
    assert any(c["lay"][0] == 0 for c in m2) and any(c["lay"][4] == 0 for c in m2) and any(c["lay"][0] == c["lay"][2] == c["lay"][4] == 0 for c in m2)
    sampled = {k: c for k, c in CASES.items() if c["model"] == "sampled"}
    assert len(sampled) == 16
    for nf in (1, 2, 4, 8):
        for cls in ("clamp", "noclamp"):
            assert sum(c["want"] == f"field_hetero_k<4,nf{nf},{cls}>" for c in sampled.values()) == 1, (nf, cls)
            assert sum(c["want"] == f"field_hetero_k<4,nf{nf},{cls},layers>" for c in sampled.values()) == 1, (nf, cls)
    assert {c["G"] for c in sampled.values()} == {1, 3, 8}
    for group in (m2, list(sampled.values())):
        assert {c["out"] for c in group} == set(OUTPUTS) and {c["apod"] for c in group} == set(APODS) and {c["rho"] for c in group} == {True, False}
        assert {c["foci"][1] for c in group} >= {3, 5, 11}                  # ragged last tiles of foci
    assert {c["n"][0] for c in CASES.values()} == {12, 13, 18, 25} and {c["n"][1] for c in CASES.values()} == {10, 16, 21, 33}
    for c in CASES.values():
        assert np.prod(c["n"]) * nz_of(c) <= 25000 and COUNTS[c["arr"]] <= 400 and c["foci"][1] <= 11


def test_table_follows_the_host_rules():
    assert {name: len(array(name)[0]) for name in COUNTS} == COUNTS
    for cid, case in CASES.items():
        xs, ys, zs = grid(case)
        pos = array(case["arr"])[0]
        cvol, avol, _ = medium(case)
        a0, nA, gap, nB, top = case["lay"]
        declared = [] if case["form"] == "uniform" else list(range(a0, a0 + nA)) + list(range(a0 + nA + gap, a0 + nA + gap + nB))
        assert nontrivial_planes(cvol, avol) == declared, cid
        if declared:
            assert (pos[:, 2] * 1e-3 < zs[declared[0]]).all(), cid           # every element strictly below the first non-trivial plane
            skull = cvol[:, :, declared] != C if case["form"] != "absorb" else avol[:, :, declared] != 0
            assert (skull.sum(axis=2).std() > 0), cid                          # laterally varying: the bilinear look-ups matter
        assert (fm.distance_class(pos, xs, ys, zs) == "clamp") == (case["cls"] == "clamp"), cid
        assert plan_rule(case) == (case["want"], case["seq"]), (cid, plan_rule(case), case["want"], case["seq"])
        eu, ev = (pos[:, 0] * 1e-3 - xs[0]) / (xs[1] - xs[0]), (pos[:, 1] * 1e-3 - ys[0]) / (ys[1] - ys[0])
        if case["ext"] == "half":                                              # EXACTLY on the threshold of the INSIDE rule, on both sides and both axes
            assert eu.min() == 0.5 and eu.max() == len(xs) - 1.5 and ev.min() == 0.5 and ev.max() == len(ys) - 1.5, cid
        elif case["ext"] == "inside":
            assert eu.min() >= 0.7 and eu.max() <= len(xs) - 1.7 and ev.min() >= 0.7 and ev.max() <= len(ys) - 1.7, cid
        else:
            assert eu.min() < 0 or eu.max() > len(xs) - 1, cid


def test_every_row_reaches_its_prefix_in_the_real_decision():
    """Without a GPU: the real decision (olxplan::decide_variant, through tools/plan_query.cpp) names, for every row, the nf and the prefix the GPU tests
    wait for.  What olx_field_set_medium establishes before it asks -- marched or sampled, the one-sum form, the non-trivial planes and their layers --
    comes from the restated host rules (plan_rule, nontrivial_planes); the decision adds the foci per launch tile and the clamp class, and names them."""
    for cid, case in CASES.items():
        pos, _, size = array(case["arr"])
        prefix, _ = plan_rule(case)
        planes = nontrivial_planes(*medium(case)[:2])
        runs = np.split(np.array(planes), np.flatnonzero(np.diff(planes) != 1) + 1) if planes else []
        layers = sum(-(-len(r) // case["G"]) for r in runs) if "layers" in prefix else 0
        d, ap = steering(cid)
        line = plan_query.variant(pos * 1e-3, size[:, 0] * size[:, 1] * 1e-6, d, ap, *grid(case), F0, C, RHO, P0, OUTPUTS[case["out"]],
                                  medium=(prefix.startswith("field_hmarch_k"), "one-sum" in prefix, len(planes), layers, case["G"]))
        assert line.split(">")[0] + ">" == case["want"], (cid, line, case["want"])
        assert f"nf{NF_OF(case['foci'][1])}," in line and f"({len(planes)} non-trivial planes" in line, (cid, line)


# ---- the references: computed once per (case, focus), shared, read-only ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def steering(cid):
    case = CASES[cid]
    pos, ori, _ = array(case["arr"])
    steer = [bo.beamform(pos * 1e-3, ori, f, C, apod=case["apod"]) for f in fm.foci_of(case)]
    return np.array([s[0] for s in steer]), np.array([s[1] for s in steer])


def reference(case, f, delays, ap):
    """The kernel's own fp64 definition on the float32 volumes the library receives."""
    pos, _, size = array(case["arr"])
    xs, ys, zs = grid(case)
    cvol, avol, _ = medium(case)
    sig, ab = co.medium_terms(cvol.astype(np.float64), avol.astype(np.float64), C, F0)
    dmin = 0.5 * min(xs[1] - xs[0], ys[1] - ys[0], zs[1] - zs[0])
    area = size[:, 0] * size[:, 1] * 1e-6
    if case["model"] == "sampled":
        return co.field_on_grid_hetero(xs, ys, zs, sig, ab, pos * 1e-3, area, delays[f], ap[f], F0, C, P0, dmin=dmin, planes_per_layer=case["G"])
    return co.field_hetero_march(xs, ys, zs, sig, ab, pos * 1e-3, area, delays[f], ap[f], F0, C, P0, dmin=dmin)


def test_references_alone():
    """Every case's fp64 reference (its last focus): finite, a positive maximum, and visibly different from the homogeneous field."""
    for cid, case in CASES.items():
        d, ap = steering(cid)
        f = len(d) - 1
        ref = reference(case, f, d, ap)
        pos, _, size = array(case["arr"])
        xs, ys, zs = grid(case)
        homog = co.field_on_grid(xs, ys, zs, pos * 1e-3, size[:, 0] * size[:, 1] * 1e-6, d[f], ap[f], F0, C, P0, dmin=0.5 * min(xs[1] - xs[0], ys[1] - ys[0], zs[1] - zs[0]))
        mx = np.abs(ref).max()
        assert np.isfinite(ref).all() and mx > 0, cid
        diff = np.abs(ref - homog).max() / mx
        if case["form"] == "uniform":
            assert diff <= 1e-12, (cid, diff)
        else:
            assert diff > 0.05, (cid, diff)


# ---- GPU: every case against its oracle ---------------------------------------------------------------------------------------------------------------
def measure(ctx, case, label, want=True, slab=None, refs=None, model=None, no_texels=False):
    """Plan (whole grid or the x-slab), set the medium, launch, fetch the case's outputs of every focus and compare them with the oracle over the full
    volume at the project's gates.  Returns (variant string after the launch, worst error per output, fetched volumes, oracle volumes)."""
    pos, ori, size = array(case["arr"])
    pos_m, area, d, ap = setup_ctx(ctx, pos, ori, size, fm.foci_of(case), apod=case["apod"])
    xs, ys, zs = grid(case)
    cvol, avol, rvol = medium(case)
    outputs = OUTPUTS[case["out"]]
    h = (xs[1] - xs[0], ys[1] - ys[0], zs[1] - zs[0])
    ctx.field_plan((xs[0], ys[0], zs[0]), h, (len(xs), len(ys), len(zs)), F0, C, RHO, P0,
                   flags=sum({"pmag": nat.OUT_PMAG, "intensity": nat.OUT_INTENSITY, "complex": nat.OUT_COMPLEX}[o] for o in outputs), slab=slab)
    ctx.field_set_medium(cvol, avol, rvol if case["rho"] else None, planes_per_layer=case["G"], model=model or case["model"])
    planned = ctx.field_variant()
    if want:
        assert planned.startswith(case["want"]), (label, planned, case["want"])
    ctx.field_launch()
    name = ctx.field_variant()
    if want and case["seq"]:
        seq = sequence(case["ext"], FORMS[case["form"]], case["lay"], no_texels=no_texels)
        assert name.startswith(case["want"]) and name.endswith(seq), (label, name, seq)
    sl = slice(None) if slab is None else slice(slab[0], slab[0] + slab[1])
    rho_c = (rvol if case["rho"] else RHO) * cvol.astype(np.float64)          # the voxel's own rho c (rho_ref where no density volume is given)
    worst = dict.fromkeys(outputs, 0.0)
    vols, refs_out = [], []
    for f in range(d.shape[0]):
        out = ctx.field_fetch(f, want=outputs)
        ref = refs[f] if refs is not None else reference(case, f, d, ap)
        vols.append(out); refs_out.append(ref)
        mx = np.abs(ref).max()
        iref = 1e-4 * np.abs(ref) ** 2 / (2 * rho_c); imx = iref.max()
        assert np.isfinite(ref).all() and mx > 0, (label, f)
        ref = ref[sl]; iref = iref[sl]
        for o in outputs:
            assert out[o].shape == ref.shape and out[o].dtype == (np.complex64 if o == "complex" else np.float32), (label, o)
            err = {"pmag": lambda: np.abs(out[o] - np.abs(ref)).max() / mx, "complex": lambda: np.abs(out[o] - ref).max() / mx,
                   "intensity": lambda: np.abs(out[o] - iref).max() / imx}[o]()
            worst[o] = max(worst[o], float(err)) if np.isfinite(err) else np.inf
    print(f"HMATRIX {label} | {name} | " + " ".join(f"{o}={worst[o]:.2e}" for o in outputs))
    for o, tol in (("pmag", HET_TOL_P), ("complex", 3 * TOL_P), ("intensity", TOL_I)):
        assert worst.get(o, 0.0) <= tol, (label, name, o, worst)
    ctx.sync()
    return name, worst, vols, refs_out


def _env(monkeypatch, case=None, no_texels=False):
    for v in ("OLX_FIELD_VARIANT", "OLX_MARCH_FUSE", "OLX_MARCH_FUSE_TI", "OLX_MARCH_SUMS", "OLX_MARCH_NO_TEXELS"):
        monkeypatch.delenv(v, raising=False)
    if case and case.get("pin"):
        monkeypatch.setenv("OLX_MARCH_SUMS", "2")
    if no_texels:
        monkeypatch.setenv("OLX_MARCH_NO_TEXELS", "1")


@pytest.mark.gpu
@pytest.mark.parametrize("cid", CASES_2M + CASES_2H)
def test_hetero_matrix_case_matches_oracle(ctx, cid, monkeypatch):
    _env(monkeypatch, CASES[cid])
    measure(ctx, CASES[cid], cid)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [next(k for k in CASES_2M if CASES[k]["seq"].startswith(f"; 2m: {side},") and "texel" in CASES[k]["seq"]) for side in ("inside", "border")])
def test_texel_lookups_equal_the_plain_lookups(ctx, cid, monkeypatch):
    """The texel cells hold copies of the same floats and the interpolation code is shared: OLX_MARCH_NO_TEXELS changes the launch sequence, not one bit."""
    case = CASES[cid]
    _env(monkeypatch, case)
    name, _, tex, refs = measure(ctx, case, cid + " texels")
    _env(monkeypatch, case, no_texels=True)
    name2, _, plain, _ = measure(ctx, case, cid + " plain", refs=refs, no_texels=True)
    assert "texel" in name and "texel" not in name2, (name, name2)
    for f in range(len(tex)):
        for o in OUTPUTS[case["out"]]:
            assert np.array_equal(tex[f][o], plain[f][o]), (cid, f, o, float(np.abs(tex[f][o] - plain[f][o]).max()))


@pytest.mark.gpu
def test_one_sum_and_pinned_two_sum_forms_agree_with_the_oracle(ctx, monkeypatch):
    """The same two-material medium through the one-sum form and, under OLX_MARCH_SUMS=2, the two-sum form: two evaluations of one definition."""
    case = CASES["2m-one-nf4-400el"]
    _env(monkeypatch)
    name1, _, one, refs = measure(ctx, case, "forms one-sum")
    pinned = dict(case, form="pin2", pin=True, want=case["want"].replace(",one-sum", ""), seq=sequence(case["ext"], False, case["lay"]))
    _env(monkeypatch, pinned)
    name2, _, two, _ = measure(ctx, pinned, "forms two-sum", refs=refs)
    assert "one-sum" in name1 and "one-sum" not in name2 and "texel" in name1 and "texel" not in name2, (name1, name2)
    for f in range(len(one)):
        mx = np.abs(refs[f]).max()
        assert np.abs(one[f]["pmag"] - two[f]["pmag"]).max() / mx <= 2 * HET_TOL_P, f


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["sampled", "marched", "auto"])
def test_uniform_medium_equals_the_homogeneous_field(ctx, model, monkeypatch):
    """A medium that is set but uniform (no non-trivial plane): every model reduces to the homogeneous Rayleigh sum (co.field_on_grid)."""
    case = CASES["2m-edge-uniform-medium"]
    _env(monkeypatch)
    pos, _, size = array(case["arr"])
    xs, ys, zs = grid(case)
    d, ap = steering("2m-edge-uniform-medium")
    refs = [co.field_on_grid(xs, ys, zs, pos * 1e-3, size[:, 0] * size[:, 1] * 1e-6, d[f], ap[f], F0, C, P0, dmin=0.5 * min(xs[1] - xs[0], ys[1] - ys[0], zs[1] - zs[0]))
            for f in range(len(d))]
    name = measure(ctx, case, f"uniform {model}", want=model != "sampled", model=model, refs=refs)[0]
    assert name.startswith("field_hetero_k<4,nf2,clamp> (0 non-trivial planes)" if model == "sampled" else "field_hmarch_k<nf2,clamp>"), name


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["2m-nf8-two-border-noclamp", "2m-one-nf4-400el"])
def test_x_slabs_tile_the_volume_bit_for_bit(ctx, cid, monkeypatch):
    """Three x-slabs of unequal width, cuts at no multiple of the 4-row tile: the writers march the whole lateral grid, the slab's voxels are the
    whole-grid launch's, bit for bit -- a two-sum case, and a one-sum case with the texel launch."""
    case = CASES[cid]
    _env(monkeypatch, case)
    assert ("texel x1" in case["seq"]) == ("one-sum" in case["want"])
    _, _, whole, refs = measure(ctx, case, cid + " whole")
    nx = case["n"][0]
    cuts = (0,) + {12: (3, 7), 13: (3, 7), 18: (5, 11), 25: (6, 15)}[nx] + (nx,)
    parts = [measure(ctx, case, f"{cid} slab {b}+{e - b}", slab=(b, e - b), refs=refs)[2] for b, e in zip(cuts[:-1], cuts[1:])]
    assert all(c % 4 for c in cuts[1:-1]) and len({e - b for b, e in zip(cuts[:-1], cuts[1:])}) == 3
    for f in range(len(whole)):
        for o in OUTPUTS[case["out"]]:
            assert np.array_equal(np.concatenate([p[f][o] for p in parts], axis=0), whole[f][o]), (cid, f, o)


@pytest.mark.gpu
def test_seeded_sweep_over_the_default_models(ctx, monkeypatch):
    """SWEEP_DRAWS random combinations of the table's axes, no pin, no expected string: whatever the library picks must pass the gate."""
    _env(monkeypatch)
    rng = np.random.default_rng(SWEEP_SEED)
    arrs = ["one", "m7x9", "flat8", "bowl10", "m10x13"]
    seen = []
    for q in range(SWEEP_DRAWS):
        arr = arrs[rng.integers(len(arrs))]
        cls = str(rng.choice(["noclamp", "clamp"]))
        a0 = 9 if (arr == "bowl10" and cls == "clamp") else int(rng.integers(3, 8))
        case = dict(arr=arr, foci=("generic", int(rng.choice([1, 2, 3, 5, 8, 11]))), seed=int(rng.integers(1000)), n=(int(rng.choice([12, 13, 18])), int(rng.choice([10, 16, 21]))),
                    lay=(a0, int(rng.integers(1, 5)), int(rng.integers(0, 4)), int(rng.integers(1, 4)), int(rng.choice([0, 1, 2, 3, 15, 16, 17]))), cls=cls,
                    ext=str(rng.choice(["inside", "border"])), form=str(rng.choice(["two", "three", "absorb", "lossless"])), out=str(rng.choice(sorted(OUTPUTS))),
                    apod=APODS[rng.integers(3)], rho=bool(rng.integers(2)), model=str(rng.choice(["auto", "auto", "sampled"])), G=1, want=None, seq=None)
        name = measure(ctx, case, f"sweep-{q}", want=False)[0]
        seen.append(name.split(">")[0] + (">" + name.split(";")[1].split(",")[0] if "; 2m:" in name else ">"))
    assert len(set(seen)) >= 3, seen
