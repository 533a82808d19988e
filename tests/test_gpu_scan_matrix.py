"""Parity matrix of the analysis scans (k_small.hip.h, launched from olx.hip) against the fp64 / longdouble oracle of tests/scan_oracle.py, on
UPLOADED synthetic volumes whose values are chosen from the oracle's own mask: every asserted number depends on one specific voxel decision
(a voxel within 1e-8 of a mask surface, a voxel exactly on it, the first plane above zmin, the extreme voxels an index box must contain, the
last 1 - 3 voxels of a z row).  One table (CASES) names per row the entry point, the frame, the row length, the focus count and whether an
intensity is uploaded; forms_of restates the host dispatch of olx.hip and says which kernel forms a row reaches.

Frames: identity_dyadic (origin, focus multiples of the spacing 2^-10 m, A = [I | -focus], aspect 1: every product and sum is exact in fp64, so
d == r and z == zmin hold exactly -- the tie cases, zero ambiguous voxels), rotated_far_origin (origin (0.2503, -0.3107, 0.4001) m, spacing
(0.5, 0.4, 0.6) mm, focus at voxel (11.3, 9.6, 13.2), A from get_focus_matrix with the effective origin (0.24, -0.30, 0), aspect (1, 1, 5), radii
1.5 / 2.5 mm: the worst cancellation the fp32 pre-test is built for), edge_focus (the ellipsoid is cut by three grid faces: the box clips),
outside_focus (empty mask: peaks 0, moments 0, no error) and thin (n = (3, 1, 3), (5, 4, 1), (6, 5, 3): nz < 4).

Gates (derived, not tuned):
 * peaks, the aggregate's max |p|, the weighted volume and its peaks: maxima of fp32 values the test uploaded or fetched -- BIT equality.
 * scaled |p| = float32(p64 s32): the kernel's one fp32 product is the correctly rounded exact product -- bit equality.
 * scaled intensity: s s (one rounding, 2^-24 relative) then the product (one rounding, half an ulp of the result): within 1.5 fp32 ulp of the
   fp64 product I s32^2.
 * mean intensity: F - 1 fp32 additions of non-negative terms (each 2^-24 of a partial sum <= the total), the rounding of 1 / F and the final
   product: |got - ref| <= (F + 1) 2^-24 ref, ref = the fp64 mean of the fetched scaled values.
 * moments: fp64 sums of N terms in some order: |got - ref| <= 4 N 2^-53 sum|term| (2 N for the summation in any order, one rounding of every
   product p x and of x = o + i h, doubled); N and the sum from the oracle.  S0 of an all-ones volume is the exact mask cardinality.
 * samples: the kernel and the oracle form the same fp64 trilinear sum in a possibly different order (relative 1e-15), then one rounding:
   within 1 fp32 ulp of the fp64 value cast to fp32.  Beam bounds are pure index logic on samples that are voxel values exactly.

Tests without a GPU: coverage (the table reaches every kernel form, both sides of F = 8 / 9, every tail length, every op, the size caps), the
oracle alone (ambiguous share, exact ties, trilinear vs SciPy, the builders' promises) and sensitivity (radius x (1 +- 1e-7), '<' swapped with
'<=', zmin moved by one plane, an index box shrunk by one voxel on any face, one row tail dropped, F = 9 averaged with 1 / 8: each changes the
expected result of the rows that name it).

Known hole: volumes past 2^24 quads, where quad_decode's float reciprocal estimate is under the most stress, need a 256 MB-per-focus upload and
do not fit a seconds-long test."""
import functools
import types

import numpy as np
import pytest

from openlifu_amd.plan.solution_analysis import get_focus_matrix
import scan_oracle as so
from scan_oracle import AMB, IN, ON, OUT

H = 2.0 ** -10
MAX_N, MAX_UPLOAD = (24, 24, 28), 64
CENTROID_FACTOR = np.float32(10 ** (-3 / 20))
BEAM_FACTORS = tuple(10 ** (-db / 20) for db in (3, 6))
K_SPIKES = 8
PERT0 = dict(radius=1.0, swap=False, zshift=0, box=None, tail=False, denom=None)
PERTURBATIONS = {"radius+": dict(radius=1 + 1e-7), "radius-": dict(radius=1 - 1e-7), "swap": dict(swap=True), "zmin": dict(zshift=1),
                 "tail": dict(tail=True), "denom": dict(denom=8), **{f"box{j}": dict(box=j) for j in range(6)}}
REQUIRED_FORMS = {"field_masked_peak_k[quad]", "field_masked_peak_k[scalar]", "field_masked_peak_box_k", "field_analysis_peaks_k<stored>",
                  "field_analysis_peaks4_k<stored>", "field_masked_moments_k", "field_masked_moments_box_k", "field_weighted_sum_k<stored>",
                  "field_weighted_sum_peak_k<stored>[quad]", "field_weighted_sum_peak_k<stored>[scalar]",
                  "field_scale_agg_analyze_k<quad,stored>", "field_scale_agg_analyze_k<rowq,stored>", "field_scale_agg_analyze_k<quad,derive>",
                  "field_scale_agg_analyze_k<rowq,derive>", "field_scale_k", "field_scale_aggregate_k<stored>", "field_aggregate_k<stored>[quad]",
                  "field_aggregate_k<stored>[scalar]", "analysis_cutoffs_k", "field_sample_k", "field_sample_lines_k", "beam_bounds_k"}


# ---- the case table --------------------------------------------------------------------------------------------------------------------------------
def _row(entry, frame, F=1, nz=None, n=None, inten=True, ops=(), zmins=(None,), radius="main", tuned=False, names=(), planned=None):
    """One row.  entry: the entry point(s) the row drives; names: the perturbations of the sensitivity test the row must feel."""
    c = dict(entry=entry, frame=frame, F=F, nz=nz, n=n, inten=inten, ops=tuple(ops), zmins=tuple(zmins), radius=radius, tuned=tuned,
             names=tuple(names), planned=planned)
    shape = "x".join(str(v) for v in n) if n else (f"nz{nz}" if nz else "")
    c["id"] = "-".join(str(v) for v in (entry, frame, shape, f"F{F}", "I" if inten else "noI", radius if entry == "peak" else "",
                                        "tuned" if tuned else "", "".join(o or "all" for o in ops)) if v != "")
    return c


BOX = tuple(f"box{j}" for j in range(6))
IN_OPS, OUT_OPS = ("<", "<="), (">", ">=", None)
ON_PLANE, BELOW, ABOVE = "on_plane", "below_grid", "above_grid"
CASES = [
    # 1. field_masked_peak, '<' and '<=': the box kernel
    _row("peak", "identity_dyadic", F=3, ops=IN_OPS, zmins=(None, ON_PLANE), names=("radius+", "radius-", "swap", "zmin") + BOX),
    _row("peak", "rotated_far_origin", F=3, nz=28, ops=IN_OPS, zmins=(None, "frame"), names=("zmin",) + BOX),
    _row("peak", "rotated_far_origin", F=1, nz=27, ops=IN_OPS, radius="side", tuned=True, inten=False, names=("radius+",) + BOX),
    _row("peak", "edge_focus", F=1, nz=28, ops=IN_OPS, zmins=(None, "frame"), names=BOX),
    _row("peak", "edge_focus", F=3, nz=25, ops=IN_OPS, inten=False, names=BOX),
    _row("peak", "outside_focus", F=1, nz=28, ops=IN_OPS, zmins=(None, "frame")),
    _row("peak", "thin", n=(3, 1, 3), ops=IN_OPS, zmins=(None, "frame"), inten=False),
    _row("peak", "thin", n=(5, 4, 1), ops=IN_OPS, inten=False),
    _row("peak", "thin", n=(6, 5, 3), F=3, ops=IN_OPS, zmins=(None, "frame"), names=BOX),
    # 2. field_masked_peak, '>' / '>=' / none: the whole-volume kernel (quads at nz % 4 == 0, scalar otherwise)
    _row("peak", "identity_dyadic", F=3, ops=OUT_OPS, zmins=(None, ON_PLANE, BELOW, ABOVE), names=("radius+", "radius-", "swap", "zmin")),
    _row("peak", "identity_dyadic", n=(16, 12, 15), F=1, ops=OUT_OPS, zmins=(ON_PLANE,), inten=False, names=("swap", "zmin")),
    _row("peak", "rotated_far_origin", F=3, nz=28, ops=OUT_OPS, zmins=(None, "frame"), radius="side", names=("zmin",)),
    _row("peak", "rotated_far_origin", F=1, nz=28, ops=OUT_OPS, tuned=True, names=("radius-",)),
    _row("peak", "rotated_far_origin", F=1, nz=27, ops=OUT_OPS, zmins=("frame",), tuned=True, inten=False, names=("radius-", "zmin")),
    _row("peak", "rotated_far_origin", F=1, nz=26, ops=(">",), zmins=("frame",), inten=False),
    _row("peak", "rotated_far_origin", F=1, nz=25, ops=(">=",), zmins=("frame",), inten=False),
    _row("peak", "edge_focus", F=1, nz=28, ops=OUT_OPS, zmins=("frame",)),
    _row("peak", "outside_focus", F=1, nz=28, ops=OUT_OPS),
    _row("peak", "thin", n=(3, 1, 3), ops=OUT_OPS, zmins=("frame",), inten=False),
    _row("peak", "thin", n=(5, 4, 1), ops=OUT_OPS, inten=False),
    # 3. field_analysis_peaks: the scalar six-peak kernel
    _row("six", "identity_dyadic", F=3, names=("radius+", "radius-", "swap", "zmin")),
    _row("six", "rotated_far_origin", F=3, nz=28, tuned=True, names=("radius+", "radius-", "zmin")),
    _row("six", "rotated_far_origin", F=1, nz=27, tuned=True, names=("radius+", "radius-")),
    _row("six", "edge_focus", F=1, nz=26, tuned=True),
    _row("six", "outside_focus", F=1, nz=25),
    _row("six", "thin", n=(6, 5, 3), F=3),
    # 4. solution_analyze, scale=None and scale=[...]: the fused pass (F <= 8) and the separate path (F = 9)
    *[_row("analyze", "rotated_far_origin", F=F, nz=nz, tuned=True, names=("radius+", "radius-", "zmin") + (("tail",) if nz % 4 else ()) + (("denom",) if F == 9 else ()))
      for F, nz in ((1, 28), (3, 27), (8, 26), (9, 25), (8, 28), (9, 28), (9, 27), (3, 25))],
    _row("analyze", "identity_dyadic", F=8, names=("radius+", "radius-", "swap", "zmin") + BOX),
    _row("analyze", "edge_focus", F=3, nz=27, tuned=True, names=BOX),
    _row("analyze", "outside_focus", F=1, nz=28),
    _row("analyze", "thin", n=(3, 1, 3), F=1),
    _row("analyze", "thin", n=(5, 4, 1), F=9),
    _row("analyze", "thin", n=(6, 5, 3), F=8),
    # 5. field_masked_moments: the whole-volume kernel
    _row("moments", "identity_dyadic", F=3, inten=False, names=("radius+",)),
    _row("moments", "rotated_far_origin", F=3, nz=28, inten=False),
    _row("moments", "rotated_far_origin", F=1, nz=27, tuned=True, inten=False, names=("radius-",)),
    _row("moments", "edge_focus", F=1, nz=25, inten=False),
    _row("moments", "outside_focus", F=1, nz=28, inten=False),
    _row("moments", "thin", n=(5, 4, 1), inten=False),
    # 6. field_sample
    _row("sample", "rotated_far_origin", nz=28), _row("sample", "thin", n=(3, 1, 3), inten=False), _row("sample", "thin", n=(5, 4, 1), inten=False),
    # 7. beam bounds through solution_analyze
    _row("beam", "identity_dyadic", F=3),
    # 8. the streaming kernels where the scalar tail meets the float4 body: odd voxel count, a multiple of 4
    *[_row("stream", "thin", n=n, F=F, inten=inten) for n in ((5, 3, 7), (4, 3, 4)) for F, inten in ((3, True), (9, True), (3, False))],
    # 9. planned (not uploaded): the DERIVE forms and a slab's x_begin in P.ox
    _row("planned", "planned", F=3, n=(24, 24, 16), planned=(5, 14)), _row("planned", "planned", F=3, n=(24, 24, 15), planned=(7, 12)),
]
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)


def rows(entry):
    return [pytest.param(c, id=c["id"]) for c in CASES if c["entry"] == entry]


def forms_of(c):
    """The kernel forms a row reaches: the host dispatch of olx.hip restated (olx_field_masked_peak, olx_solution_analyze_begin,
    olx_field_scale_aggregate and the streaming entry points)."""
    nx, ny, nz = shape_of(c)
    vox, F, e = nx * ny * nz, c["F"], c["entry"]
    D = "derive" if e == "planned" else "stored"
    out = set()
    if e == "peak":
        for op in c["ops"]:
            out.add("field_masked_peak_box_k" if op in IN_OPS else f"field_masked_peak_k[{'quad' if nz % 4 == 0 else 'scalar'}]")
        if c["inten"]:
            out.add(f"field_weighted_sum_k<{D}>")
    if e == "six":
        out.add(f"field_analysis_peaks_k<{D}>")
    if e in ("analyze", "beam", "planned"):
        peaks = f"field_analysis_peaks4_k<{D}>" if nz % 4 == 0 else f"field_analysis_peaks_k<{D}>"
        wsp = f"field_weighted_sum_peak_k<{D}>[{'quad' if nz % 4 == 0 and vox % 4 == 0 else 'scalar'}]"
        out |= {peaks, wsp, "analysis_cutoffs_k", "field_masked_moments_box_k", "field_masked_peak_box_k", "field_sample_lines_k", "beam_bounds_k"}   # scale=None
        if e != "beam":                                                                                                                           # scale=[...]
            if F <= 8:
                out.add(f"field_scale_agg_analyze_k<{'rowq' if nz % 4 else 'quad'},{D}>")
            else:
                out |= {f"field_scale_aggregate_k<{D}>"} if vox % 4 == 0 else {"field_scale_k", f"field_aggregate_k<{D}>[scalar]"}
    if e == "moments":
        out.add("field_masked_moments_k")
    if e == "sample":
        out.add("field_sample_k")
    if e == "stream":
        q = "quad" if vox % 4 == 0 else "scalar"
        out |= {f"field_aggregate_k<stored>[{q}]", "field_scale_k"}
        if c["inten"]:
            out |= {"field_weighted_sum_k<stored>", "field_scale_aggregate_k<stored>" if vox % 4 == 0 else "field_scale_k"}
    return out


# ---- geometry ----------------------------------------------------------------------------------------------------------------------------------------
def shape_of(c):
    if c["planned"]:
        return (c["planned"][1],) + tuple(c["n"][1:])
    if c["n"]:
        return tuple(c["n"])
    return (16, 12, 16) if c["frame"] == "identity_dyadic" else (24, 20, c["nz"])


def planned_setup(c):
    """The 8 x 8 array of test_aggregate_scale_masked_peak_and_upload, its three foci, a 1 mm grid of c["n"] voxels and an x-slab."""
    foci = np.array([[0, 0, 30e-3], [3e-3, 0, 30e-3], [0, -3e-3, 33e-3]])
    n = c["n"]
    xs = (np.arange(n[0]) - (n[0] - 1) / 2) * 1e-3
    ys = (np.arange(n[1]) - (n[1] - 1) / 2) * 1e-3
    zs = (22.0 + np.arange(n[2])) * 1e-3
    return foci, xs, ys, zs


@functools.lru_cache(maxsize=None)
def _geometry(cid):
    c = BY_ID[cid]
    F, fr, n = c["F"], c["frame"], shape_of(c)
    G = types.SimpleNamespace(n=n, F=F, exact=False, aspect=(1.0, 1.0, 5.0), r_main=1.5e-3, r_side=2.5e-3)
    k = np.arange(F)
    if fr == "identity_dyadic":
        G.exact, G.aspect, G.spacing, G.origin = True, (1.0, 1.0, 1.0), (H, H, H), (-7 * H, 3 * H, 32 * H)
        vc = np.stack([7 + k % 4, 6 - k % 2, 8 - k % 3], axis=1).astype(float)
        G.r_main, G.r_side = 3 * H, 5 * H                                  # (1, 2, 2) h and (3, 4, 0) h lie ON them
        G.zmin = G.origin[2] + 5 * H
    elif fr == "thin":
        G.spacing, G.origin, G.aspect = (1e-3, 0.8e-3, 1.2e-3), (0.01, -0.02, 0.03), (1.0, 1.0, 1.0)
        vc = (np.array(n) - 1) / 2 + 0.2 + 0.3 * np.stack([k % 3, k % 2, k % 4], axis=1)
        G.r_main, G.r_side = 1.1e-3, 1.6e-3
        G.zmin = G.origin[2] + 0.4 * G.spacing[2]
    elif fr == "planned":
        foci, xs, ys, zs = planned_setup(c)
        G.spacing, G.origin = (1e-3, 1e-3, 1e-3), (xs[0] + c["planned"][0] * 1e-3, ys[0], zs[0])
        G.r_main, G.r_side, G.zmin = 2.5e-3, 4e-3, 25.4e-3
        vc = (foci - np.array(G.origin)) / 1e-3
    else:
        G.spacing, G.origin = (0.5e-3, 0.4e-3, 0.6e-3), (0.2503, -0.3107, 0.4001)
        vc0 = {"rotated_far_origin": (11.3, 9.6, 13.2), "edge_focus": (1.2, 18.1, 2.3), "outside_focus": (-40.0, 9.6, 13.2)}[fr]
        off = np.random.default_rng(7).uniform(-2.5, 2.5, (F, 3)); off[0] = 0
        vc = np.array(vc0) + off
        G.zmin = G.origin[2] + 6.4 * G.spacing[2]
    G.foci = np.array(G.origin) + vc * np.array(G.spacing) if fr != "planned" else planned_setup(c)[0]
    if G.exact:
        G.M = [np.block([[np.eye(3), f[:, None]], [np.zeros((1, 3)), np.ones((1, 1))]]) for f in G.foci]
        G.A = np.array([np.hstack([np.eye(3), -f[:, None]]).ravel() for f in G.foci])
    else:
        eff = {"thin": (0.0, 0.0, 0.0), "planned": (0.0, 0.0, 0.0)}.get(fr, (0.24, -0.30, 0.0))
        G.M = [get_focus_matrix(f, origin=eff) for f in G.foci]
        G.A = np.array([np.linalg.inv(M)[:3].ravel() for M in G.M])
    G.d = [so.distance(G.origin, G.spacing, n, G.A[f], G.aspect) for f in range(F)]
    if c["tuned"] or fr == "planned":       # radii next to a voxel of focus 0: the mainlobe winner just inside r_main, the sidelobe winner just outside r_side
        d0 = G.d[0]
        G.r_main = so.tuned_radius(d0.ravel()[np.argmin(np.abs(d0 - G.r_main))], "in")
        G.r_side = so.tuned_radius(d0.ravel()[np.argmin(np.abs(d0 - G.r_side))], "out")
    return G


def geometry(c):
    return _geometry(c["id"])


def zmin_of(G, kind):
    hz, oz, nz = G.spacing[2], G.origin[2], G.n[2]
    return {None: None, "frame": G.zmin, ON_PLANE: oz + 5 * hz, BELOW: oz - 1.5 * hz, ABOVE: oz + (nz + 0.5) * hz}[kind]


def pert_of(name):
    return {**PERT0, **(PERTURBATIONS[name] if name else {})}


def zsel(G, zmin, pert):
    """(selected planes, ambiguous planes) of z > zmin."""
    z = None if zmin is None else zmin + pert["zshift"] * G.spacing[2]
    c = so.classify_z(G.origin[2], G.spacing[2], G.n[2], z, G.exact)
    return c == IN, c == AMB


def shrunk_box(mask, pert):
    """The index box of a mask (None: unrestricted), one voxel short on face pert["box"]."""
    if pert["box"] is None:
        return None
    box = so.bounding_box(mask)
    box[pert["box"]] += 1 if pert["box"] % 2 == 0 else -1
    return so.in_box(mask.shape, box)


SWAP = {"<": "<=", "<=": "<", ">": ">=", ">=": ">", None: None}


def near_of(G, f, r, zmin):
    """Distance of every voxel from the nearest selection surface, in voxels (ranks the builders' plantings)."""
    near = np.abs(G.d[f] - so.LD(r)).astype(np.float64) / min(G.spacing)
    if zmin is not None:
        z = so.axes([G.origin[2]], [G.spacing[2]], [G.n[2]], np.float64)[0]
        near = np.minimum(near, np.abs(z - zmin) / G.spacing[2]) if r > 0 else np.broadcast_to(np.abs(z - zmin) / G.spacing[2], near.shape)
    return near


# ---- entry points 1 / 2: field_masked_peak -----------------------------------------------------------------------------------------------------------
def peak_plan(c, pert=PERT0):
    """Per (op, zmin): the uploaded stack (per focus its graded_out volume and its one_hot spikes, built from the UNPERTURBED selection), the
    frame of every volume, the (perturbed) mask the scan of every volume runs over and the expected peaks."""
    G = geometry(c)
    r0 = G.r_main if c["radius"] == "main" else G.r_side
    plans = []
    for op in c["ops"]:
        for zk in c["zmins"]:
            zmin = zmin_of(G, zk)
            vols, A, masks, planted = [], [], [], []
            for f in range(G.F):
                sel = []
                for p in (PERT0, pert):
                    zs, za = zsel(G, zmin, p)
                    cl = so.classify(G.d[f], r0 * p["radius"], G.exact)
                    m = so.select(cl, SWAP[op] if p["swap"] else op) & zs
                    amb = ((cl == AMB) & (op is not None)) | za
                    box = shrunk_box(m, p) if op in IN_OPS else None
                    sel.append((m if box is None else m & box, amb))
                (mask, amb), (pmask, _) = sel
                near = near_of(G, f, r0 if op is not None else 0.0, zmin)
                st, vox, vals = so.one_hot(mask, near, K_SPIKES)
                vols += [so.graded_out(mask, amb, near), *st]
                planted += [0.0, *vals]
                A += [G.A[f]] * (1 + len(st)); masks += [pmask] * (1 + len(st))
            vols = np.stack(vols)
            plans.append(dict(op=op, zmin=zmin, r=r0, vols=vols, A=np.array(A), masks=masks, planted=np.array(planted, dtype=np.float32),
                              expect=np.array([so.masked_peak(v, m) for v, m in zip(vols, masks)], dtype=np.float32)))
    return plans


@pytest.mark.gpu
@pytest.mark.parametrize("c", rows("peak"))
def test_masked_peak(ctx, c):
    """graded_out gives 0 and every one_hot volume its spike, bit-equal, on |p|, on the intensity and on the weighted volume (vol_stride 0)."""
    G = geometry(c)
    for P in peak_plan(c):
        assert np.array_equal(P["expect"], P["planted"])
        S = len(P["vols"])
        inten = np.roll(P["vols"], 1, axis=0) if c["inten"] else None
        ctx.field_upload(G.origin, G.spacing, G.n, P["vols"], inten)
        got = ctx.field_masked_peak(P["A"], G.aspect, P["r"], P["op"], "pmag", zmin_m=P["zmin"])
        assert np.array_equal(got, P["expect"]), (P["op"], P["zmin"], got, P["expect"])
        if c["inten"]:
            got = ctx.field_masked_peak(P["A"], G.aspect, P["r"], P["op"], "intensity", zmin_m=P["zmin"])
            want = np.array([so.masked_peak(v, m) for v, m in zip(inten, P["masks"])], dtype=np.float32)      # (rolled: a focus' first volume is its neighbour's last spike)
            assert np.array_equal(got, want), (P["op"], P["zmin"], "intensity", got, want)
            for k in (0, S - 1):                               # weights e_k: the weighted volume IS intensity volume k; every frame scans that ONE volume
                w = np.zeros(S); w[k] = 1.0
                ctx.field_weighted_intensity(w)
                assert np.array_equal(ctx.field_weighted_fetch(), inten[k])
                got = ctx.field_masked_peak(P["A"], G.aspect, P["r"], P["op"], "weighted_intensity", zmin_m=P["zmin"])
                want = np.array([so.masked_peak(inten[k], m) for m in P["masks"]], dtype=np.float32)
                assert np.array_equal(got, want), (P["op"], P["zmin"], "weighted", k, got, want)


# ---- entry points 3 / 4 / 9: the six peaks and the one-call analysis ------------------------------------------------------------------------------
def _pick(cond, near, taken=()):
    idx = np.flatnonzero(cond)
    idx = idx[~np.isin(idx, [t for t in taken if t is not None])]
    return None if idx.size == 0 else int(idx[np.argmin(near.ravel()[idx])])


def planted(c):
    """|p| and intensity [F, nx, ny, nz] whose three masks have DIFFERENT winners, each next to a surface.  |p|: a (mainlobe winner, 5) is the
    in-mask voxel nearest r_main, a2 just outside it is larger (9, the global winner); b (sidelobe winner, 7) is the voxel nearest outside r_side,
    b2 just inside it is larger (8); the mainlobe's extreme voxels (what its index box must contain) lie above the -3 dB cut-off, the rest of it on
    both sides.  Intensity: the same plantings, and the sidelobe / global winner (40) sits in the FIRST plane above zmin.  In both, a voxel outside
    r_side in the last plane that is not above zmin is the largest of all."""
    G = geometry(c)
    rng = np.random.default_rng(11)
    zok, zamb = zsel(G, G.zmin, PERT0)
    zv, zav = np.broadcast_to(zok, G.n), np.broadcast_to(zamb, G.n)
    plane = np.broadcast_to(np.arange(G.n[2]), G.n)
    k1 = int(np.argmax(zok)) if zok.any() else -9            # first plane above zmin
    k0 = int(np.flatnonzero(~zok & ~zamb).max()) if (~zok & ~zamb).any() else -9
    ps, ws = [], []
    for f in range(G.F):
        cm, cs = so.classify(G.d[f], G.r_main, G.exact), so.classify(G.d[f], G.r_side, G.exact)
        main = cm == IN
        nm, ns = np.abs(G.d[f] - so.LD(G.r_main)).astype(float), np.abs(G.d[f] - so.LD(G.r_side)).astype(float)
        a = _pick(main, nm)
        a2 = _pick((cm == OUT) & (cs == IN) & zv, nm)
        b = _pick((cs == OUT) & zv, ns)
        b2 = _pick((cs == IN) & (cm == OUT) & zv, ns, (a2,))
        first = _pick((cs == OUT) & (plane == k1), -ns, (b,))
        below = _pick((cs == OUT) & (plane == k0), -ns)
        ext = []
        if main.any():
            idx = np.flatnonzero(main); co = np.unravel_index(idx, G.n)
            ext = [int(idx[pick(co[ax])]) for ax in range(3) for pick in (np.argmin, np.argmax)]
        for out, vals in ((ps, (5.0, 9.0, 7.0, 8.0, None, 20.0)), (ws, (6.0, 10.0, 30.0, 8.5, 40.0, 50.0))):
            v = rng.uniform(0.1, 1.0, G.n)
            v[main] = rng.uniform(1.0, 4.9, int(main.sum()))
            v.ravel()[ext] = 4.95
            for vox, val in zip((a, a2, b, b2, first, below), vals):
                if vox is not None and val is not None:
                    v.ravel()[vox] = val
            v[(cm == AMB) | (cs == AMB) | zav] = 0.0
            if G.exact:
                v[(cm == ON) | (cs == ON)] = 15.0               # ON a surface: neither '<' nor '>' selects it (the global peak does)
            out.append(v.astype(np.float32))
    return np.stack(ps), np.stack(ws)


def weights_of(F):
    w = 0.5 + 0.25 * (np.arange(F) % 5)
    if F >= 3:
        w[2] = 0.0
    return w


def scales_of(F):
    s = 0.75 + 0.3 * (np.arange(F) % 4)
    if F >= 3:
        s[1] = 0.0
    return s


def analyze_expect(c, p, i, wvol, pert=PERT0):
    """What solution_analyze reports for the volumes p, i [F, ...] and the weighted volume: the oracle's masks, maxima and fp64 sums."""
    G = geometry(c)
    rm, rs = G.r_main * pert["radius"], G.r_side * pert["radius"]
    zok, _ = zsel(G, G.zmin, pert)
    zv = np.broadcast_to(zok, G.n)
    E = dict(peaks=np.zeros((G.F, 6), np.float32), ita_main=np.zeros(G.F, np.float32), moments=np.zeros((G.F, 4)), gate=np.zeros((G.F, 4)),
             cut=np.zeros(G.F, np.float32), main=[])
    for f in range(G.F):
        cm, cs = so.classify(G.d[f], rm, G.exact), so.classify(G.d[f], rs, G.exact)
        main, side = so.select(cm, "<=" if pert["swap"] else "<"), so.select(cs, ">=" if pert["swap"] else ">")
        E["peaks"][f] = so.six_peaks(p[f], i[f], main, side, zv)
        box = shrunk_box(main, pert)
        mb = main if box is None else main & box                # the moments and the weighted volume's mainlobe peak run over the index box
        E["cut"][f] = E["peaks"][f, 0] * CENTROID_FACTOR        # fp32 x fp32 -> fp32, as analysis_cutoffs_k documents
        E["moments"][f], E["gate"][f] = so.moments(p[f], mb, E["cut"][f], G.origin, G.spacing)
        E["ita_main"][f] = so.masked_peak(wvol, mb)
        E["main"].append(mb)
    E["ita_global"] = so.masked_peak(wvol, zv)
    E["pmax"], E["imean"] = so.aggregate(p, i, pert["denom"])
    if pert["tail"]:                                            # the tail of row (0, 0) never written
        E["pmax"] = E["pmax"].copy(); E["pmax"][0, 0, G.n[2] & ~3:] = -1.0
    return E


def line_points(G, grid_lines=False):
    """(offsets per axis, pts [F, n0 + n1 + n2, 3]).  grid_lines (dyadic frame): voxel centres along the grid axes, the x line with a repeated
    zero offset, the z line leaving the grid at both ends."""
    if grid_lines:
        offs = [np.array([-5, -4, -3, -2, -1, 0, 0, 0, 1, 2, 3, 4]) * H, np.arange(-3, 4) * H, np.arange(-12, 13) * H]
    else:
        offs = [np.linspace(-s * 2 * G.r_main, s * 2 * G.r_main, m) for s, m in zip(G.aspect, (9, 7, 11))]
    pts = []
    for M in G.M:
        rows_ = []
        for a, off in enumerate(offs):
            loc = np.zeros((len(off), 4)); loc[:, a] = off; loc[:, 3] = 1.0
            rows_.append((loc @ M.T)[:, :3])
        pts.append(np.concatenate(rows_))
    return offs, np.array(pts)


def expected_bounds(G, p, peaks, offs, pts):
    """[F, 3, 2, 2] from the oracle's samples; also the smallest distance of a sample from a cut-off in fp32 ulp (a precondition of the comparison)."""
    out = np.zeros((G.F, 3, 2, 2), dtype=np.int32)
    margin = np.inf
    for f in range(G.F):
        smp = so.trilinear(p[f], G.origin, G.spacing, pts[f]).astype(np.float32)
        start = 0
        for a, off in enumerate(offs):
            n_le = int(np.count_nonzero(off <= 0)); ge = np.nonzero(off >= 0)[0]
            for lv, fac in enumerate(BEAM_FACTORS):
                cut = np.float32(np.float64(peaks[f, 0]) * fac)
                seg = smp[start:start + len(off)]
                out[f, a, lv] = so.beam_bounds(seg, cut, n_le, int(ge[0]) if ge.size else len(off))
                fin = seg[np.isfinite(seg)]
                if fin.size and cut > 0:
                    margin = min(margin, float(np.min(np.abs(fin.astype(np.float64) - cut) / so.ulp32(cut))))
            start += len(off)
    return out, margin


def check_report(c, rep, p, i, wvol, offs, pts):
    G = geometry(c)
    E = analyze_expect(c, p, i, wvol)
    print(c["id"], "peaks", rep["peaks"].tolist(), "ita", rep["ita_main"].tolist(), rep["ita_global"])
    assert np.array_equal(rep["peaks"], E["peaks"]), (rep["peaks"], E["peaks"])
    assert np.array_equal(rep["ita_main"], E["ita_main"]) and np.float32(rep["ita_global"]) == E["ita_global"]
    for f in range(G.F):        # precondition: no mainlobe value within 2 fp32 ulp of the -3 dB cut-off
        v = p[f][E["main"][f]].astype(np.float64)
        assert v.size == 0 or E["cut"][f] == 0 or np.min(np.abs(v - E["cut"][f])) > 2 * so.ulp32(E["cut"][f])
    err = np.abs(rep["moments"] - E["moments"])
    print(c["id"], "moments err / gate", (err / np.maximum(E["gate"], 1e-300)).max() if err.size else 0)
    assert np.all(err <= E["gate"]), (rep["moments"], E["moments"], E["gate"])
    want, margin = expected_bounds(G, p, rep["peaks"], offs, pts)
    assert margin > 2.0, margin          # interpolated samples may differ by an ulp: none may sit next to a cut-off
    assert np.array_equal(rep["bounds"], want), (rep["bounds"], want)
    return E


def check_scaled(F, p0, i0, s, p1, i1, pm, im):
    """The gates of the scaling and of the aggregate, on the fetched volumes."""
    assert np.array_equal(p1, so.scale_p(p0, s))
    if i0 is not None:
        ref = so.scale_i64(i0, s)
        err = np.abs(i1.astype(np.float64) - ref) / np.maximum(so.ulp32(ref.astype(np.float32)), 1e-300)
        print("scaled intensity: max error", err.max(), "ulp (gate 1.5)")
        assert err.max() <= 1.5
    if pm is not None:
        assert np.array_equal(pm, so.aggregate(p1)[0])
    if im is not None:
        ref = so.aggregate(p1, i1)[1]
        err = np.abs(im - ref)
        print("mean intensity: max error / gate", (err / np.maximum((F + 1) * 2.0 ** -24 * ref, 1e-300)).max())
        assert np.all(err <= (F + 1) * 2.0 ** -24 * ref)


@pytest.mark.gpu
@pytest.mark.parametrize("c", rows("six"))
def test_analysis_peaks_scalar_kernel(ctx, c):
    G = geometry(c)
    p, i = planted(c)
    ctx.field_upload(G.origin, G.spacing, G.n, p, i)
    got = ctx.field_analysis_peaks(G.A, G.aspect, G.r_main, G.r_side, G.zmin)
    E = analyze_expect(c, p, i, np.zeros(G.n, np.float32))
    print(c["id"], got.tolist())
    assert np.array_equal(got, E["peaks"]), (got, E["peaks"])
    if c["frame"] in ("rotated_far_origin", "identity_dyadic"):
        assert all(len(set(E["peaks"][f, 0::2])) == 3 for f in range(G.F))       # three masks, three winners


@pytest.mark.gpu
@pytest.mark.parametrize("c", rows("analyze"))
def test_solution_analyze(ctx, c):
    G = geometry(c)
    p, i = planted(c)
    w = weights_of(G.F)
    offs, pts = line_points(G)
    for s in (None, scales_of(G.F)):
        ctx.field_upload(G.origin, G.spacing, G.n, p, i)
        rep = ctx.solution_analyze(G.A, w, G.aspect, G.r_main, G.r_side, G.zmin, line_pts=pts, line_offsets=offs, scale=s)
        got = ctx.field_fetch_all()
        wv = ctx.field_weighted_fetch()
        assert np.array_equal(wv, so.weighted(got["intensity"], w))
        if s is None:
            assert np.array_equal(got["pmag"], p) and np.array_equal(got["intensity"], i)
        else:
            pm, im = ctx.aggregate_fetch()
            check_scaled(G.F, p, i, s, got["pmag"], got["intensity"], pm, im)
        check_report(c, rep, got["pmag"], got["intensity"], wv, offs, pts)


@pytest.mark.gpu
@pytest.mark.parametrize("c", rows("planned"))
def test_planned_slab_derived_intensity(ctx, c):
    """A planned (not uploaded) x-slab: the scans derive the intensity from |p| (the DERIVE forms) and P.ox carries the slab's x_begin."""
    from test_gpu_field import C, F0, P0, RHO, setup_ctx
    from conftest import synthetic_array
    G = geometry(c)
    foci, xs, ys, zs = planned_setup(c)
    pos, ori, size = synthetic_array(8, 8, 4.0)
    setup_ctx(ctx, pos, ori, size, foci)
    w = weights_of(G.F)
    offs, pts = line_points(G)
    for s in (None, [1.25, 0.5, 2.0]):
        ctx.field_plan((xs[0], ys[0], zs[0]), (1e-3,) * 3, c["n"], F0, C, RHO, P0, slab=c["planned"])
        ctx.field_launch()
        before = ctx.field_fetch_all()
        assert before["pmag"].shape[1:] == G.n
        rep = ctx.solution_analyze(G.A, w, G.aspect, G.r_main, G.r_side, G.zmin, line_pts=pts, line_offsets=offs, scale=s)
        got = ctx.field_fetch_all()
        wv = ctx.field_weighted_fetch()
        assert np.array_equal(wv, so.weighted(got["intensity"], w))
        if s is not None:
            pm, im = ctx.aggregate_fetch()
            check_scaled(G.F, before["pmag"], None, s, got["pmag"], got["intensity"], pm, im)
        E = check_report(c, rep, got["pmag"], got["intensity"], wv, offs, pts)
        assert all(m.any() for m in E["main"]) and np.all(E["peaks"][:, 0] > 0)


# ---- entry point 5: field_masked_moments ---------------------------------------------------------------------------------------------------------------
def moments_plan(c, pert=PERT0):
    """(volumes [2 F], frames, cut-offs, expected sums, gates): per focus an all-ones volume with cut-off 0 (S0 = the mask's cardinality) and a
    graded one whose cut-off lies between two values planted one fp32 ulp apart on the in-mask voxels nearest the surface (strict '>')."""
    G = geometry(c)
    r = G.r_main
    rng = np.random.default_rng(5)
    vols, A, cuts, exp, gate, counts = [], [], [], [], [], []
    for f in range(G.F):
        cl = so.classify(G.d[f], r, G.exact)
        mask, amb = so.select(cl, "<"), cl == AMB
        near = near_of(G, f, r, None)
        ones = np.ones(G.n, np.float32); ones[amb] = 0
        gr = rng.uniform(1.0, 2.0, G.n).astype(np.float32); gr[amb] = 0
        if G.exact:
            gr[cl == ON] = 1.9
        lo = _pick(mask, near); hi = _pick(mask, near, (lo,))
        if lo is not None:
            gr.ravel()[lo] = 1.5
        if hi is not None:
            gr.ravel()[hi] = np.nextafter(np.float32(1.5), np.float32(2))
        pm = so.select(so.classify(G.d[f], r * pert["radius"], G.exact), "<")
        for v, cut in ((ones, 0.0), (gr, 1.5)):
            e, g = so.moments(v, pm, cut, G.origin, G.spacing)
            vols.append(v); A.append(G.A[f]); cuts.append(cut); exp.append(e); gate.append(g)
        counts.append(int(pm.sum()))
    return np.stack(vols), np.array(A), np.array(cuts, np.float32), np.array(exp), np.array(gate), counts


@pytest.mark.gpu
@pytest.mark.parametrize("c", rows("moments"))
def test_masked_moments(ctx, c):
    G = geometry(c)
    vols, A, cuts, exp, gate, counts = moments_plan(c)
    ctx.field_upload(G.origin, G.spacing, G.n, vols)
    got = ctx.field_masked_moments(A, G.aspect, G.r_main, cuts)
    print(c["id"], "S0", got[:, 0].tolist(), "counts", counts)
    assert np.array_equal(got[0::2, 0], np.array(counts, dtype=np.float64))       # one misclassified voxel changes S0 by 1
    assert np.all(np.abs(got - exp) <= gate), (got, exp, gate)


# ---- entry point 6: field_sample -----------------------------------------------------------------------------------------------------------------------
def sample_points(G):
    """(pts [P, 3], kind [P]): random interior points, points exactly on voxels (the last plane of every axis among them), points 5e-10 (n - 1)
    voxels outside a face (kind "edge": the edge value) and points half a voxel outside (kind "out": NaN)."""
    rng = np.random.default_rng(3)
    o, h, n = np.array(G.origin), np.array(G.spacing), np.array(G.n)
    pts, kind = [o + rng.uniform(0, 1, (200, 3)) * (n - 1) * h], ["in"] * 200
    vox = np.array([[0, 0, 0], n - 1, [n[0] - 1, 0, 0], [0, n[1] - 1, 0], [0, 0, n[2] - 1], (n - 1) // 2, *rng.integers(0, n, (20, 3))])
    pts.append(o + vox * h); kind += ["voxel"] * len(vox)
    for a in range(3):
        for side in (0, 1):
            base = rng.uniform(0, 1, (4, 3)) * (n - 1)
            e = base.copy(); e[:, a] = (n[a] - 1) * side + (2 * side - 1) * 5e-10 * max(n[a] - 1, 1)
            x = base.copy(); x[:, a] = (n[a] - 1) * side + (2 * side - 1) * 0.5
            pts += [o + e * h, o + x * h]; kind += ["edge"] * 4 + ["out"] * 4
    return np.concatenate(pts), np.array(kind)


@pytest.mark.gpu
@pytest.mark.parametrize("c", rows("sample"))
def test_field_sample(ctx, c):
    G = geometry(c)
    rng = np.random.default_rng(9)
    p = rng.uniform(0.5, 2.0, (2,) + G.n).astype(np.float32)
    i = rng.uniform(0.5, 2.0, (2,) + G.n).astype(np.float32) if c["inten"] else None
    pts, kind = sample_points(G)
    ctx.field_upload(G.origin, G.spacing, G.n, p, i)
    for which, vols in (("pmag", p), ("intensity", i)):
        if vols is None:
            continue
        for f in range(2):
            got = ctx.field_sample(f, pts, which)
            ref = so.trilinear(vols[f], G.origin, G.spacing, pts)
            assert np.all(np.isnan(got[kind == "out"])) and not np.any(np.isnan(got[kind != "out"]))
            ok = kind != "out"
            err = np.abs(got[ok].astype(np.float64) - ref[ok].astype(np.float32)) / so.ulp32(ref[ok])
            print(c["id"], which, f, "max sample error", err.max(), "ulp (gate 1)")
            assert err.max() <= 1.0


# ---- entry point 7: beam bounds ------------------------------------------------------------------------------------------------------------------------
def beam_volumes(c):
    """Dyadic frame: the focus voxel carries the mainlobe peak 4; along the grid x line through it sit a value EQUAL to the -3 dB cut-off (not below),
    one an ulp under it (below -3 dB only) and one an ulp under the -6 dB cut-off; the y line never crosses (-1, -1); the z line leaves the grid."""
    G = geometry(c)
    vc = np.rint((G.foci - np.array(G.origin)) / H).astype(int)
    c3, c6 = (np.float32(4.0 * f) for f in BEAM_FACTORS)
    p = np.full((G.F,) + G.n, 0.5, dtype=np.float32)
    for f, (x, y, z) in enumerate(vc):
        p[f, :, y, z] = 4.0; p[f, x, :, z] = 4.0; p[f, x, y, :] = 4.0
        p[f, x - 3, y, z] = c3
        p[f, x - 4, y, z] = np.nextafter(c3, np.float32(0))
        p[f, x + 2, y, z] = np.nextafter(c6, np.float32(0))
        p[f, x, y, z + 3] = np.nextafter(c3, np.float32(0))
        p[f, x, y, 0] = 0.0
    return p, (p * p * np.float32(0.25)).astype(np.float32), vc


@pytest.mark.gpu
@pytest.mark.parametrize("c", rows("beam"))
def test_beam_bounds_on_grid_lines(ctx, c):
    G = geometry(c)
    p, i, vc = beam_volumes(c)
    offs, pts = line_points(G, grid_lines=True)
    ctx.field_upload(G.origin, G.spacing, G.n, p, i)
    rep = ctx.solution_analyze(G.A, weights_of(G.F), G.aspect, G.r_main, G.r_side, G.zmin, line_pts=pts, line_offsets=offs)
    assert np.array_equal(rep["peaks"][:, 0], np.full(G.F, 4.0, np.float32))
    want, _ = expected_bounds(G, p, rep["peaks"], offs, pts)
    print(c["id"], rep["bounds"].tolist())
    assert np.array_equal(rep["bounds"], want), (rep["bounds"], want)
    # x line, offsets (-5 .. -1, 0, 0, 0, 1 .. 4) h: -3 dB below at -4 h (index 1; the value AT the cut-off, index 2, is not) and at +2 h (index 9);
    # -6 dB no crossing on the negative side; y line none at all
    assert np.array_equal(want[:, 0], np.tile([[[1, 9], [-1, 9]]], (G.F, 1, 1))) and np.all(want[:, 1] == -1)


# ---- entry point 8: the streaming kernels ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("c", rows("stream"))
def test_streaming_aggregate_scale_weighted(ctx, c):
    G = geometry(c)
    F = G.F
    rng = np.random.default_rng(13)
    p = rng.uniform(0.0, 3.0, (F,) + G.n).astype(np.float32); p[rng.uniform(size=p.shape) < 0.1] = 0
    i = (rng.uniform(0.0, 3.0, p.shape).astype(np.float32) if c["inten"] else None)
    s, w = scales_of(F), weights_of(F)
    up = lambda: ctx.field_upload(G.origin, G.spacing, G.n, p, i)      # noqa: E731
    fetch = lambda: ctx.field_fetch_all(want=("pmag", "intensity") if c["inten"] else ("pmag",))      # noqa: E731
    up()
    pm, im = ctx.field_aggregate(want_intensity=c["inten"])
    check_scaled(F, p, i, np.ones(F), p, i, pm, im)
    if c["inten"]:
        ctx.field_weighted_intensity(w)
        assert np.array_equal(ctx.field_weighted_fetch(), so.weighted(i, w))
    ctx.field_scale(s)
    got = fetch()
    check_scaled(F, p, i, s, got["pmag"], got.get("intensity"), None, None)
    if c["inten"]:
        up()
        ctx.field_scale_aggregate(s)
        got = fetch()
        pm, im = ctx.aggregate_fetch()
        check_scaled(F, p, i, s, got["pmag"], got["intensity"], pm, im)


# ---- without a GPU ---------------------------------------------------------------------------------------------------------------------------------------
def test_table_reaches_every_form_and_edge():
    reached = set().union(*(forms_of(c) for c in CASES))
    assert REQUIRED_FORMS <= reached, REQUIRED_FORMS - reached
    an = [c for c in CASES if c["entry"] == "analyze"]
    assert {1, 3, 8, 9} <= {c["F"] for c in an}
    for tail in (0, 1, 2, 3):       # every tail length on both sides of F = 8 / 9 is too much; every tail on the fused side, 0 / 1 / 3 on the separate one
        assert any(shape_of(c)[2] % 4 == tail and shape_of(c)[2] >= 4 and c["F"] <= 8 for c in an), tail
        assert any(shape_of(c)[2] % 4 == tail and shape_of(c)[2] >= 4 for c in CASES if c["entry"] == "peak" and set(c["ops"]) & set(OUT_OPS)), tail
    assert {shape_of(c)[2] % 4 for c in an if c["F"] == 9} >= {0, 1, 3}
    assert {shape_of(c) for c in an if shape_of(c)[2] < 4} == {(3, 1, 3), (5, 4, 1), (6, 5, 3)}
    assert {op for c in CASES for op in c["ops"]} == set(so.OPS)
    assert {c["inten"] for c in CASES if c["entry"] in ("peak", "stream")} == {True, False}
    for c in CASES:
        n = shape_of(c)
        assert all(a <= b for a, b in zip(n, MAX_N)), c["id"]
        if c["entry"] == "peak":
            assert all(len(P["vols"]) <= MAX_UPLOAD for P in peak_plan(c)), c["id"]
        assert c["F"] <= MAX_UPLOAD


@pytest.mark.parametrize("c", [pytest.param(c, id=c["id"]) for c in CASES if c["entry"] != "stream"])
def test_oracle_classification(c):
    """Per case the ambiguous share is a condition: at most 2 voxels per focus and radius, exactly 0 in the tie cases and on rotated_far_origin."""
    G = geometry(c)
    for f in range(G.F):
        for r in (G.r_main, G.r_side):
            n_amb = int((so.classify(G.d[f], r, G.exact) == AMB).sum())
            assert n_amb <= 2 and (n_amb == 0 or c["frame"] not in ("identity_dyadic", "rotated_far_origin")), (c["id"], f, r, n_amb)
    for zk in set(c["zmins"]) | {"frame"}:
        assert not zsel(G, zmin_of(G, zk), PERT0)[1].any() or not G.exact
    if G.exact:         # the ties are there: (1, 2, 2) h on r_main = 3 h, (3, 4, 0) h on r_side = 5 h
        assert all((so.classify(G.d[f], r, True) == ON).sum() >= 6 for f in range(G.F) for r in (G.r_main, G.r_side))
        assert (so.classify_z(G.origin[2], H, G.n[2], zmin_of(G, ON_PLANE), True) == IN).tolist() == [False] * 6 + [True] * (G.n[2] - 6)


@pytest.mark.parametrize("c", [pytest.param(c, id=c["id"]) for c in CASES if c["entry"] in ("peak", "six", "analyze")])
def test_volumes_keep_their_promises(c):
    """What the GPU tests rely on, checked on the uploaded volumes: graded_out scans to 0 and every spike to its value; the planted volumes have
    three winners, no mainlobe value within 2 fp32 ulp of the -3 dB cut-off and no line sample within 2 ulp of a beam cut-off."""
    G = geometry(c)
    if c["entry"] == "peak":
        for P in peak_plan(c):
            assert np.array_equal(P["expect"], P["planted"]) and len(P["vols"]) >= G.F
        return
    p, i = planted(c)
    E = analyze_expect(c, p, i, so.weighted(i, weights_of(G.F)))
    if c["frame"] in ("rotated_far_origin", "identity_dyadic"):
        assert all(len(set(E["peaks"][f, 0::2])) == 3 and E["peaks"][f, 0] == 5 and E["peaks"][f, 2] == 7 for f in range(G.F))
        assert np.all(E["peaks"][:, 3] == 40) and np.all(E["moments"][:, 0] > 5)
    for s in (np.ones(G.F), scales_of(G.F)):
        ps = so.scale_p(p, s)
        Es = analyze_expect(c, ps, i, np.zeros(G.n, np.float32))
        for f in range(G.F):
            v = ps[f][Es["main"][f]].astype(np.float64)
            assert v.size == 0 or Es["cut"][f] == 0 or np.min(np.abs(v - Es["cut"][f])) > 2 * so.ulp32(Es["cut"][f])
        offs, pts = line_points(G)
        assert expected_bounds(G, ps, Es["peaks"], offs, pts)[1] > 2.0


def test_oracle_rotated_far_origin_mask_sizes():
    c = next(c for c in CASES if c["frame"] == "rotated_far_origin" and c["nz"] == 28 and not c["tuned"])
    G = geometry(c)
    for r, size in ((1.5e-3, 599), (2.5e-3, 2329)):
        cl = so.classify(G.d[0], r)
        assert int((cl == IN).sum()) == size and not (cl == AMB).any()
        assert int((np.abs(G.d[0] - so.LD(r)) <= 3e-6).sum()) == 8


def test_oracle_builders_and_tuned_radius():
    c = BY_ID[next(c["id"] for c in CASES if c["entry"] == "six" and c["frame"] == "rotated_far_origin" and c["F"] == 3)]
    G = geometry(c)
    d = G.d[0]
    for r, side in ((G.r_main, IN), (G.r_side, OUT)):
        cl = so.classify(d, r)
        k = np.argmin(np.abs(d - so.LD(r)))
        assert cl.ravel()[k] == side and 5e-9 < abs(float(d.ravel()[k] / so.LD(r) - 1)) < 2e-8 and not (cl == AMB).any()
    mask, near = cl == OUT, np.abs(d - so.LD(r)).astype(float)
    g = so.graded_out(mask, cl == AMB, near)
    assert so.masked_peak(g, mask) == 0 and len(np.unique(g[~mask])) == (~mask).sum() and g.ravel()[np.argmin(np.where(mask, np.inf, near))] == g.max()
    st, vox, vals = so.one_hot(cl == IN, near, 8)
    box = so.bounding_box(cl == IN)
    ijk = np.array(np.unravel_index(vox, G.n)).T
    assert all((ijk[:, a] == box[2 * a]).any() and (ijk[:, a] == box[2 * a + 1] - 1).any() for a in range(3))
    assert [so.masked_peak(v, cl == IN) for v in st] == list(vals) and all((v != 0).sum() == 1 for v in st)


def test_oracle_trilinear_agrees_with_scipy():
    scipy_interp = pytest.importorskip("scipy.interpolate")
    G = geometry(next(c for c in CASES if c["entry"] == "sample" and c["frame"] == "rotated_far_origin"))
    vol = np.random.default_rng(1).uniform(0, 1, G.n).astype(np.float32)
    pts, kind = sample_points(G)
    ax = so.axes(G.origin, G.spacing, G.n, np.float64)
    ref = scipy_interp.RegularGridInterpolator(ax, vol.astype(np.float64), bounds_error=False, fill_value=np.nan)(pts)
    got = so.trilinear(vol, G.origin, G.spacing, pts)
    sel = (kind == "in") | (kind == "voxel")
    assert np.abs(got[sel] - ref[sel]).max() <= 1e-9 and np.all(np.isnan(got[kind == "out"])) and np.all(np.isnan(ref[kind == "out"]))
    assert not np.any(np.isnan(got[kind == "edge"]))
    assert so.beam_bounds([1, np.nan, 0.5, 2, 2, 0.4, np.nan], 1.0, 4, 3) == (2, 5) and so.beam_bounds([np.nan, 2.0], 1.0, 1, 1) == (-1, -1)


def _flat(e):
    if isinstance(e, dict):
        return np.concatenate([np.ravel(np.asarray(e[k], dtype=np.float64)) for k in ("peaks", "ita_main", "moments", "ita_global", "pmax", "imean")])
    return np.concatenate([np.ravel(np.asarray(v, dtype=np.float64)) for v in e])


def expected(c, name=None):
    """Everything the GPU tests of a row compare with, as one vector, under a perturbation of the ORACLE's parameters (volumes stay as built)."""
    pert = pert_of(name)
    if c["entry"] == "peak":
        return _flat([P["expect"] for P in peak_plan(c, pert)])
    if c["entry"] == "moments":
        return _flat(moments_plan(c, pert)[3])
    p, i = planted(c)
    return _flat(analyze_expect(c, p, i, so.weighted(i, weights_of(c["F"])), pert))


@pytest.mark.parametrize("c", [pytest.param(c, id=c["id"]) for c in CASES if c["names"]])
def test_sensitivity(c):
    base = expected(c)
    for name in c["names"]:
        assert not np.array_equal(expected(c, name), base), (c["id"], name)


def test_every_perturbation_is_named():
    assert set(PERTURBATIONS) == {n for c in CASES for n in c["names"]}
