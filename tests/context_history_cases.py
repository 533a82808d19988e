"""Probes and histories of the context-history matrix (tests/test_gpu_context_history.py runs them, tests/test_context_history_host.py keeps
the tables honest).  Nothing here touches the device at import; the case tables of the other matrices are imported where a probe needs them.

A PROBE is one complete small operation on a context -- elements, steering, settings, plan, launch, fetch -- taken from a case table that already
has an fp64 oracle, and run through that table's own runner, so a probe that returns has passed its module's gate.  It returns (variant string,
dict of arrays).  Every probe starts with neutral(): the five settings "for the plans that follow" at their defaults and no developer pin in the
environment, because most of the imported runners set only the settings their own family knows.

A HISTORY is an ordered list of steps on ONE context that ends in a probe (or in a re-plan / launch of a probe's plan); the matrix demands that the
last step gives the bits and the variant string a fresh context gives.  Steps:
    ("run", name)      a probe or one of EXTRA_RUNS (larger or differently shaped problems of the same families), results dropped
    ("set", name, on)  one of SETTINGS switched on (a non-default value) or back off
    ("act", name)      one of ACTS: another engine or a state change on the context as it stands (no new elements, no new steering)
    ("plan", probe)    the probe's set-up and olx_field_plan, no launch           (CW lattice probes only)
and the last step is one of ("probe", name), ("replan", name) -- olx_field_plan again with the probe's arguments on the elements and steering the
context holds, then launch and fetch -- ("launch", name) -- launch and fetch of the plan that stands -- or ("relaunch", name), the same after a run.

COUPLINGS names what each history is for (the numbering of DESIGN.md section 3, "The context-history matrix")."""
from __future__ import annotations

import functools
import os

import numpy as np

MAX_VOXELS, MAX_ELEMENTS, MAX_FOCI, MAX_STEPS = 24 * 20 * 28, 256, 3, 12
COUPLINGS = {1: "buffer capacity", 2: "upload caches", 3: "the re-plan shortcut", 4: "settings left set", 5: "focus knowledge",
             6: "derived and stored intensity", 7: "PII and p_max residency", 8: "other engines between plan and launch"}
SETTINGS = ("absorption", "pulse", "response", "medium_model", "layering")
ENV_PINS = ("OLX_FIELD_VARIANT", "OLX_INTENSITY_STORED", "OLX_FP8_CORRECTION", "OLX_MARCH_FUSE", "OLX_MARCH_FUSE_TI", "OLX_MARCH_SUMS", "OLX_MARCH_NO_TEXELS")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---- the case tables the probes come from (imported on first use) -----------------------------------------------------------------------------------
def _lm():
    import test_gpu_lattice_matrix as m
    return m


def _fm():
    import test_gpu_field_matrix as m
    return m


def _hm():
    import test_gpu_hetero_matrix as m
    return m


@functools.lru_cache(maxsize=None)
def lattice_cases():
    """Rows made with test_gpu_lattice_matrix's generator at the probes' sizes: an 8 x 8 array at 3 voxels pitch (2g with three foci, 2e with two), the
    16 x 16 array with one on-axis focus (2f) and with three generic foci on 24 x 20 x 28 voxels, where the e4m3 rule admits the correction products
    -- it reads the foci to do so -- and the 8 x 8 array with uniform absorption and with piston directivity in the tables.  The others are the
    histories' neighbours: the same array under another fold pattern, another pitch, other foci, a stored intensity."""
    lm = _lm()
    c, a8, p3, g = lm._case, (8, 8), (3, 3), (24, 20, 16)
    return {
        "cw_lat_2g": c("2g", a8, p3, g, "xy", foci=("generic", 3), out="pi"),
        "cw_lat_2e": c("2e", a8, p3, g, "xy", nt=1, foci=("generic", 2)),
        "cw_lat_2f": c("2f", (16, 16), p3, g, "xy", e4m3=True, foci=("axis", 1), frag=("1 row tile(s)",)),
        "cw_lat_e4m3": c("2g", (16, 16), p3, (24, 20, 28), "xy", e4m3=True, foci=("generic", 3), out="pi"),
        "cw_lat_absorb": c("2g", a8, p3, g, "xy", foci=("generic", 3), absorb=lm.ABSORB, frag=("uniform absorption in the tables",)),
        "cw_lat_dir": c("2g", a8, p3, g, "xy", foci=("generic", 3), dirv=True, out="pi", frag=("piston directivity in the tables",)),
        # neighbours
        "lat_2g_xfold": c("2g", a8, p3, g, "x", foci=("generic", 5)),                        # the grid shifted along y: the y fold is gone, other columns
        "lat_2g_pitch32": c("2g", a8, (3, 2), g, "xy", foci=("generic", 3)),                  # another pitch: another partition
        "lat_2g_other_target": c("2g", a8, p3, g, "xy", foci=("generic", 3), out="pi", seed=23),      # the same pattern of columns at other foci
        "lat_2g_stored": c("2g", a8, p3, g, "xy", foci=("generic", 3), out="pi", stored=True),
        "lat_2g_lossless_twin": c("2g", a8, p3, g, "xy", foci=("generic", 3)),           # cw_lat_absorb's plan in every argument but the absorption
    }


LATTICE_PROBES = ("cw_lat_2g", "cw_lat_2e", "cw_lat_2f", "cw_lat_e4m3", "cw_lat_absorb", "cw_lat_dir")
GENERAL_PROBES = {"cw_gen_2a": "2a-default-jittered", "cw_gen_2b": "2b-default-x", "cw_gen_2c": "2c-none-nt1-nz16"}       # rows of test_gpu_field_matrix.CASES
HETERO_PROBES = {"cw_het_2h": "2h-nf1-noclamp-G3", "cw_het_2m": "2m-nf2-two-inside-noclamp"}                               # rows of test_gpu_hetero_matrix.CASES
PULSED_PROBES = {"pulsed_plain": ("unit_tap", False), "pulsed_ring30": ("ring30", True), "pulsed_classes_9x9": ("classes_9x9", True)}   # (pulsed_response_cases row, response?)
STEER_PROBES = {"steer_a8_maxangle": ("a8", "maxangle30", 0.0, False), "steer_a8_absorb_dir": ("a8", "uniform", 5.0, True)}             # rows of test_gpu_steering.CASES
BF_PROBES = {"bf_maxangle_M": ("maxangle", 20.0, 0.0), "bf_piecewise_M": ("piecewise", 60.0, 20.0)}                         # the m8x8_jitter table of golden/g2_beamform.npz, with its matrix
STEER_MEDIUM_PROBES = {"steer_medium_e3": ("e3", "uniform", "equalize", True, "straight_ray", False, "both")}                          # a row of test_gpu_steering_medium.CASES
PULSED_MEDIUM_PROBES = {"pulsed_medium_slab16": "slab16"}                                                                            # a row of pulsed_medium_cases.CASES
MEDIUM_BF_PROBES = ("bf_solve_medium", "bf_compensated_quantize")       # the scene of test_gpu_medium_delays / test_gpu_medium_apod on 24 x 20 x 28 voxels, its first three foci, with the matrix
BF_MEDIUM_GRID = (24, 20, 28)
LATE_PROBES = {"thermal_resident": "thermal", "fullwave_lockin": "fullwave_lockin", "fullwave_aperture": "fullwave_aperture", "uploaded_analyze": "uploaded"}
FULLWAVE_LOCKIN_CASE, FULLWAVE_APERTURE_CASE = "short_axis", "edges"       # rows of fullwave_lockin_cases.LOCK_CASES / fullwave_aperture_cases.CASES
# the probes the matrix must hold, by name (tests/test_context_history_host.py): the list of the issue this matrix answers
REQUIRED_PROBES = ("cw_lat_2g", "cw_lat_2f", "cw_lat_e4m3", "cw_gen_2a", "cw_gen_2b", "cw_gen_2c", "cw_lat_absorb", "cw_gen_absorb", "cw_lat_dir", "cw_het_2h", "cw_het_2m",
                   "pulsed_plain", "pulsed_ring30", "pulsed_classes_9x9", "pulsed_medium_slab16", "bf_maxangle_M", "bf_piecewise_M", "bf_solve_medium",
                   "bf_compensated_quantize", "steer_a8_maxangle", "steer_a8_absorb_dir", "steer_medium_e3", "thermal_uploaded", "thermal_resident",
                   "fullwave_short_axis", "fullwave_lockin", "fullwave_aperture", "eikonal_short_axis", "uploaded_analyze")
# named exceptions to the size caps: the dyadic-frame row of test_gpu_scan_matrix the uploaded probe is taken from has 8 foci
CAP_EXCEPTIONS = {"uploaded_analyze": "foci"}
OTHER_PROBES = {"thermal_uploaded": "water_to_the_boundary", "fullwave_short_axis": "short_axis", "eikonal_short_axis": "short_axis"}

FAMILY = {**dict.fromkeys(LATTICE_PROBES[:4], "cw_lattice"), "cw_lat_absorb": "cw_modifier", "cw_lat_dir": "cw_modifier", "cw_gen_absorb": "cw_modifier",
          **dict.fromkeys(GENERAL_PROBES, "cw_general"), **dict.fromkeys(HETERO_PROBES, "cw_hetero"), **dict.fromkeys(PULSED_PROBES, "pulsed"),
          **dict.fromkeys(STEER_PROBES, "steer"), **dict.fromkeys(STEER_MEDIUM_PROBES, "steer_medium"), **dict.fromkeys(PULSED_MEDIUM_PROBES, "pulsed_medium"), **dict.fromkeys(BF_PROBES, "bf"), "thermal_uploaded": "thermal", "fullwave_short_axis": "fullwave",
          "eikonal_short_axis": "eikonal", **dict.fromkeys(MEDIUM_BF_PROBES, "bf_medium"), **LATE_PROBES}
PROBES = tuple(FAMILY)

# larger or differently shaped problems for the histories (rows of the same tables, run through the same runners)
EXTRA_RUNS = {
    "big_lattice": ("lattice", "2g-xy-fp16"),                     # 8 x 16 elements, 40 x 44 x 23 voxels, |p| and intensity
    "big_lattice_240el": ("lattice", "2g-x-fp16"),                # 20 x 12 elements under the x fold only, 5 foci
    "many_foci_lattice": ("lattice", "2g-xy-36col-3tiles"),       # 9 foci in three column tiles
    "big_general_400el": ("general", "2c-xy-400el-nt1-2chunks"),
    "shared_2b_64el": ("general", "2b-default-xy"),               # kernel 2b on 64 elements: d_perm / up_perm between two lattice plans
    "big_hetero": ("hetero", "2m-one-nf4-400el"),
    "steer_c16": ("steer", ("c16", "uniform", 0.0, True)),        # 256 elements, 33 x 31 x 35 voxels
    "steer_e3": ("steer", ("e3", "uniform", 0.0, False)),         # 3 elements, 9 x 7 x 11
    "steer_medium_e100": ("steer_medium", ("e100", "uniform", None, False, "direct", False, "both")),      # 100 elements on the same 9 x 7 x 11 voxels
    "pulsed_medium_64el": ("pulsed_medium", "slab64_2foci"),
    "thermal_big": ("thermal", "skull_layers_perfusion"),
    "eikonal_big": ("eikonal", "uniform_water"),
    "fullwave_other": ("fullwave", "short_axis_layered"),
}


def probe_shape(name):
    """(voxels, elements, foci) of a probe, from its case table."""
    fam = FAMILY[name]
    if name in lattice_cases():
        c = lattice_cases()[name]
        return int(np.prod(c["n"])), c["arr"][0] * c["arr"][1], len(_lm().foci_of(c))
    if name in GENERAL_PROBES or name == "cw_gen_absorb":
        fm = _fm()
        c = fm.CASES[GENERAL_PROBES.get(name, "2a-default-jittered")]
        return int(np.prod(c["n"])), len(fm.array(c["arr"])[0]), c["foci"][1]
    if fam == "cw_hetero":
        hm = _hm()
        c = hm.CASES[HETERO_PROBES[name]]
        return int(np.prod(c["n"])) * hm.nz_of(c), hm.COUNTS[c["arr"]], c["foci"][1]
    if fam == "pulsed":
        import pulsed_response_cases as pc
        k = pc.case(PULSED_PROBES[name][0])
        return int(np.prod(k.n)), len(k.pos_m), len(k.delays)
    if fam == "steer":
        import test_gpu_steering as ts
        el, _, _, n = ts.geometry(STEER_PROBES[name][0])
        return int(np.prod(n)), len(el["pos"]), 0
    if fam == "steer_medium":
        import test_gpu_steering_medium as tsm
        el, _, _, n = tsm.geometry(STEER_MEDIUM_PROBES[name][0])
        return int(np.prod(n)), len(el["pos"]), 0
    if fam == "pulsed_medium":
        import pulsed_medium_cases as pmc
        k = pmc.case(PULSED_MEDIUM_PROBES[name])
        return int(np.prod(k.n)), len(k.pos_m), len(k.foci_m)
    if fam == "bf_medium":
        return int(np.prod(BF_MEDIUM_GRID)), 64, 3
    if name == "thermal_resident":
        return probe_shape("cw_lat_2g")
    if name == "fullwave_lockin":
        import fullwave_cases as fc
        return int(np.prod(fc.CASES[FULLWAVE_LOCKIN_CASE]["n"])), 0, 0
    if name == "fullwave_aperture":
        import fullwave_aperture_cases as ac
        return int(np.prod(ac.CASES[FULLWAVE_APERTURE_CASE]["n"])), len(ac.CASES[FULLWAVE_APERTURE_CASE]["A"]), 0
    if name == "uploaded_analyze":
        G = __import__("test_gpu_scan_matrix").geometry(uploaded_row())
        return int(np.prod(G.n)), 0, int(G.F)
    if fam == "bf":
        import test_gpu_bf as tb
        g = np.load(os.path.join(GOLDEN, "g2_beamform.npz"))
        return 0, len(tb._table(g, "m8x8_jitter")[0]), min(MAX_FOCI, len(g["m8x8_jitter_targets_m"]))
    if fam == "thermal":
        import test_gpu_thermal as tt
        c = tt.CASES[OTHER_PROBES[name]]
        return int(np.prod(c["shape"])), 0, c["foci"]
    mod = __import__("fullwave_cases" if fam == "fullwave" else "eikonal_cases")
    return int(np.prod(mod.CASES[OTHER_PROBES[name]]["n"])), 0, 0


# ---- runners -----------------------------------------------------------------------------------------------------------------------------------------
def neutral(ctx, mp, settings=True):
    """The probe's own set-up of what no imported runner sets for it: no developer pin and, with ``settings``, every setting "for the plans that
    follow" at its default."""
    for v in ENV_PINS:
        mp.delenv(v, raising=False)
    if not settings:
        return
    ctx.field_absorption(0.0)
    ctx.field_pulse(0.0, 0.0, 0)
    ctx.field_pulse_response()
    ctx._chk(ctx._lib.olx_field_medium_model(ctx._h, 0))
    ctx._chk(ctx._lib.olx_field_medium_layering(ctx._h, 1))


def _volumes(vols):
    return {f"{o}[{f}]": v for f, d in enumerate(vols) for o, v in d.items()}


def _run_lattice(ctx, mp, case, label):
    name, _, vols = _lm().run_lcase(ctx, case, label, mp)
    return name, _volumes(vols)


def _run_general(ctx, mp, cid, label, absorb=0.0):
    fm = _fm()
    case = fm.CASES[cid]
    if not absorb:
        name, _, vols, _ = fm.run_case(ctx, case, label)
        return name, _volumes(vols)
    pos, ori, size = fm.array(case["arr"])        # the jittered array under uniform absorption: the per-pair modifier kernel (field_accum_dir_k)
    pos_m, area, d, ap = fm.setup_ctx(ctx, pos, ori, size, fm.foci_of(case), apod=case["apod"])
    ctx.field_absorption(absorb)
    try:
        name, _, vols, _ = fm.measure(ctx, *fm.grid(case), pos_m, area, d, ap, fm.OUTPUTS["pi"], want_variant="field_accum_dir_k<4,", label=label,
                                      fragments=("uniform absorption",), absorption=absorb)
    finally:
        ctx.field_absorption(0.0)
    return name, _volumes(vols)


def _run_hetero(ctx, mp, cid, label):
    hm = _hm()
    hm._env(mp, hm.CASES[cid])
    name, _, vols, _ = hm.measure(ctx, hm.CASES[cid], label)
    return name, _volumes(vols)


def _run_pulsed(ctx, mp, row, label):
    import pulsed_response_cases as pc
    import test_gpu_pulsed_response as tp
    name, response = row
    vox = pc.case(name).trace_voxels()
    out, tr = pc.run_device(ctx, name, response=response, trace=vox)
    dev = tp.deviations(name, out, tr, vox)          # the gates of test_response_kernel_matches_oracle (the unit tap's oracle IS the plain burst's)
    print(f"[history] {label}: " + ", ".join(f"{k} {v:.3e}" for k, v in dev.items()))
    assert dev["p_max"] <= tp.P_TOL and dev["p_min"] <= tp.P_TOL and dev["pii"] <= tp.PII_TOL and dev["trace"] <= tp.TRACE_TOL and dev["intensity"] <= tp.I_TOL, (label, dev)
    if response:
        tp.check_trace_invariants(name, out, tr, vox)
    variant = out.pop("variant")
    return variant, dict(out, trace=tr)


def _run_steer(ctx, mp, case, label):
    import test_gpu_steering as ts
    pf, na = ts.run(ctx, case)
    ts.check(case, pf, na)
    return "", {"P": pf, "n_active": na}


def _run_steer_medium(ctx, mp, case, label):
    import test_gpu_steering_medium as tsm
    pf, na = tsm.run(ctx, case)
    tsm.check(case, pf, na)
    return "", {"P": pf, "n_active": na}


def _run_pulsed_medium(ctx, mp, name, label):
    import pulsed_medium_cases as pmc
    import test_gpu_pulsed_medium as tpm
    k = pmc.case(name)
    out, variant = tpm.launch(ctx, k)           # test_pulsed_medium_kernel_matches_oracle's launch and gate
    tpm.check_gate(out, [k.oracle(f) for f in range(len(k.foci_m))], z=k.ss.astype(np.float64) * tpm.RHO, label=label)
    return variant, out


def _run_bf(ctx, mp, apod, label):
    from openlifu_amd import _native as nat
    import test_gpu_bf as tb
    g = np.load(os.path.join(GOLDEN, "g2_beamform.npz"))
    key = "m8x8_jitter"
    ctx.set_elements(*tb._table(g, key))
    kind = {"maxangle": nat.APOD_MAXANGLE, "piecewise": nat.APOD_PIECEWISE}[apod[0]]
    F = MAX_FOCI                                  # the table's first three foci
    d, a = ctx.bf_solve(g[key + "_targets_m"][:F], 1500.0, matrix=g[key + "_M"], apod_kind=kind, p0=apod[1], p1=apod[2])
    ref = g[f"{key}_delays_params"][:F]
    assert np.abs(d - ref).max() <= 1e-12 * ref.max(), label                                   # test_g2_all_foci_one_launch's gates
    if apod[0] == "maxangle":
        assert np.array_equal(a, g[f"{key}_apod_maxangle20"][:F]), label
    else:
        assert np.abs(a - g[key + "_apod_pwl_60_20"][:F]).max() <= 1e-12, label
    return "", {"delays": d, "apod": a}


def _medium_bf_scene(ctx):
    """Elements (the jittered 8 x 8 array), medium volumes, grid, three foci (a voxel, a voxel inside the skull, a point off the voxels) and the matrix
    of test_delays_match_oracle / test_apodization_matches_oracle."""
    import test_gpu_medium_delays as md
    origin, spacing, (xs, ys, zs) = md._grid(BF_MEDIUM_GRID, 1e-3, 4e-3)
    cvol, avol = md._skull(xs, ys, zs)
    pos_m, area = md._elements(ctx)
    foci = np.array([[xs[12], ys[10], zs[22]], [xs[3], ys[17], zs[11]], [1.3e-3, -2.7e-3, 25.35e-3]])
    M = np.eye(4)
    M[:3, 3] = [0.4e-3, -0.3e-3, -0.5e-3]
    return md, origin, spacing, cvol, avol, pos_m, area, foci, M


def _run_bf_medium(ctx, mp, label):
    from openlifu_amd import _native as nat
    import medium_delay_oracle as mo
    md, origin, spacing, cvol, _, pos_m, _, foci, M = _medium_bf_scene(ctx)
    ctx.bf_set_medium(cvol, origin, spacing, BF_MEDIUM_GRID, md.C)
    d, a = ctx.bf_solve_medium(foci, md.C, matrix=M, apod_kind=nat.APOD_MAXANGLE, p0=50.0)
    ref = mo.delays(pos_m, foci, cvol, origin, spacing, md.C, M=M)
    assert np.abs(d - ref).max() <= 1e-12, (label, np.abs(d - ref).max())                      # test_delays_match_oracle's gate
    assert np.abs(ref - mo.delays(pos_m, foci, None, origin, spacing, md.C, M=M)).max() > 1e-7   # the medium matters here
    return "", {"delays": d, "apod": a}


def _run_bf_compensated_quantize(ctx, mp, label):
    from openlifu_amd import _native as nat
    from oracle import bf_oracle as bo
    import medium_apod_oracle as ao
    md, origin, spacing, _, avol, pos_m, area, foci, M = _medium_bf_scene(ctx)
    ctx.bf_set_attenuation(avol, origin, spacing, BF_MEDIUM_GRID, md.F0)
    d0, b = ctx.bf_solve(foci, md.C, matrix=M, apod_kind=nat.APOD_MAXANGLE, p0=50.0)
    d, a = ctx.bf_solve_compensated(foci, md.C, matrix=M, apod_kind=nat.APOD_MAXANGLE, p0=50.0, mode="matched", spreading=True)
    _, h, _ = ao.arrival(pos_m, foci, avol, origin, spacing, md.F0, area=area, M=M)
    ref = ao.compensate(b, h, "matched")
    assert np.abs(a - ref).max() <= 1e-12 and np.array_equal(a == 0, b == 0) and np.array_equal(d, d0), label      # test_apodization_matches_oracle's gates
    assert np.abs(a - b).max() > 1e-3
    got = ctx.bf_quantize(10e6, 13)                                           # ... then the hand-off numbers of that resident table, bit-exact
    want = bo.tx_quantize(d, a)
    assert all(np.array_equal(g, w) for g, w in zip(got, want)) and not got[3].any(), label
    return "", {"delays": d, "apod": a, "ticks": got[0], "apod_off": got[1], "max_apod": got[2], "overflow": got[3]}


def _run_thermal_resident(ctx, mp, label):
    """The thermal model on the RESIDENT intensity of the CW lattice probe before it (derived there: olx_thermal_source materialises it), against
    the thermal oracle fed the intensity that probe fetched."""
    import test_gpu_thermal as tt
    import thermal_oracle as to
    variant, cw = run(ctx, mp, "cw_lat_2g", label=label + ":cw")
    origin, h, n = _plan_args(lattice_cases()["cw_lat_2g"])[0][:3]
    F = 3
    inten = np.stack([cw[f"intensity[{f}]"] for f in range(F)])
    rho, cp, kap, att = tt.WATER
    alpha = float(tt._np_m(att))
    steps = 40
    dt = 0.5 * to.ftcs_bound(rho, cp, kap, h, n, 0.0)
    sched = tt.pulsed_sched(F, dt, steps, 0.3 * dt, 0.7 * dt, count=6 * F + 1, train=0.0, trains=steps // (6 * F + 1) + 1)
    pts = np.array([np.ravel_multi_index(tuple(v // 2 for v in n), n), 0, int(np.prod(n)) - 1])
    ctx.thermal_plan(origin, h, n, rho, cp, kap, alpha)
    ctx.thermal_schedule(*sched, points=pts)
    ctx.thermal_source(F, None)
    ctx.thermal_run(dt, 37.0)
    got = ctx.thermal_fetch()
    tt.check_gate(got, to.run(rho, cp, kap, alpha, inten, h, *sched, dt, steps, baseline=37.0, perfusion=0.0, points=pts))
    return variant, dict(cw, rise=got[0], cem43=got[1], traces=got[2])


def _run_fullwave_lockin(ctx, mp, label):
    import fullwave_cases as fc
    import fullwave_lockin_cases as lc
    import test_gpu_fullwave_lockin as tl
    name = FULLWAVE_LOCKIN_CASE
    window = tl.windows(fc.CASES[name]["steps"])["last_third"]
    table = lc.receiver_csr(name, lc.receivers(name))
    rec, got = lc.run_device(ctx, name, window, table)
    tl.check(got, lc.lockin_reference(name, window, table), label)            # test_matches_oracle's gates (volume and receiver sums)
    out = dict(zip(("p_max", "p_min", "psq", "trace", "C", "S", "C_r", "S_r"), tuple(rec) + tuple(got)))
    return "", {k: v for k, v in out.items() if v is not None}


def _run_fullwave_aperture(ctx, mp, label):
    import fullwave_aperture_cases as ac
    import test_gpu_fullwave_aperture as ta
    got = ac.run_device(ctx, FULLWAVE_APERTURE_CASE)
    ta.check_gate(got, ac.reference(FULLWAVE_APERTURE_CASE), label)          # test_runs_match_oracle's gate
    return "", {k: v for k, v in zip(("p_max", "p_min", "psq", "trace"), got) if v is not None}


def uploaded_row():
    """The dyadic-frame row of test_gpu_scan_matrix's solution_analyze entry."""
    sm = __import__("test_gpu_scan_matrix")
    return next(c for c in sm.CASES if c["entry"] == "analyze" and c["frame"] == "identity_dyadic")


def _run_uploaded(ctx, mp, label):
    """olx_field_upload of the row's planted volumes, solution_analyze with a scaling (scale_aggregate and weighted_intensity inside it), every volume
    fetched after it: test_solution_analyze's gates.  The moments are fp64 atomic sums: returned under a key that says so."""
    import test_gpu_scan_matrix as sm
    c = uploaded_row()
    G = sm.geometry(c)
    p, i = sm.planted(c)
    w, s = sm.weights_of(G.F), sm.scales_of(G.F)
    offs, pts = sm.line_points(G)
    ctx.field_upload(G.origin, G.spacing, G.n, p, i)
    rep = ctx.solution_analyze(G.A, w, G.aspect, G.r_main, G.r_side, G.zmin, line_pts=pts, line_offsets=offs, scale=s)
    got = ctx.field_fetch_all()
    wv = ctx.field_weighted_fetch()
    pm, im = ctx.aggregate_fetch()
    assert np.array_equal(wv, sm.so.weighted(got["intensity"], w)), label
    sm.check_scaled(G.F, p, i, s, got["pmag"], got["intensity"], pm, im)
    sm.check_report(c, rep, got["pmag"], got["intensity"], wv, offs, pts)
    return "", {"pmag": got["pmag"], "intensity": got["intensity"], "weighted": wv, "agg_pmag": pm, "agg_intensity": im, "peaks": np.asarray(rep["peaks"]),
                "ita_main": np.asarray(rep["ita_main"]), "ita_global": np.array([rep["ita_global"]], dtype=np.float32), "bounds": np.asarray(rep["bounds"]),
                ATOMIC + "moments": np.asarray(rep["moments"], dtype=np.float64)}


ATOMIC = "atomic:"      # prefix of an output summed with fp64 atomics: equal from run to run within rtol = atol = 1e-12, not bit for bit
_LATE_RUNNERS = {"bf_solve_medium": _run_bf_medium, "bf_compensated_quantize": _run_bf_compensated_quantize, "thermal_resident": _run_thermal_resident,
                 "fullwave_lockin": _run_fullwave_lockin, "fullwave_aperture": _run_fullwave_aperture, "uploaded_analyze": _run_uploaded}


@functools.lru_cache(maxsize=None)
def _thermal_args(name):
    import test_gpu_thermal as tt
    import thermal_oracle as to
    cs = tt.CASES[name]
    shape, h, F = cs["shape"], cs["h"], cs["foci"]
    medium = tt.layered(shape) if cs["layered"] else tt.WATER
    centres = [tuple(s // 2 + d for s in shape) for d in (0, 2, -3)][:F]
    inten = tt.gaussian_sources(shape, centres, 2.0, peak=200.0 if cs["layered"] else 2000.0)
    rho, cp, kap, _ = (np.broadcast_to(np.asarray(v, dtype=np.float64), shape) for v in medium)
    dt = 0.5 * to.ftcs_bound(rho, cp, kap, h, shape, cs["perfusion"])
    sched = tt.pulsed_sched(F, dt, cs["steps"], 0.3 * dt, 0.7 * dt, count=6 * F + 1, train=0.0, trains=cs["steps"] // (6 * F + 1) + 1)
    pts = np.array([np.ravel_multi_index(c, shape) for c in centres] + [0, int(np.prod(shape)) - 1]) if cs["points"] else None
    return shape, h, medium, inten, sched, dt, cs["steps"], cs["perfusion"], pts


def _run_thermal(ctx, mp, name, label):
    import test_gpu_thermal as tt
    shape, h, medium, inten, sched, dt, steps, perf, pts = _thermal_args(name)         # test_thermal_kernel_matches_oracle's scene, through its run_case and gate
    got, ref = tt.run_case(ctx, shape, h, medium, inten, sched, dt, steps, perfusion=perf, points=pts)
    tt.check_gate(got, ref)
    return "", {"rise": got[0], "cem43": got[1], "traces": got[2]}


def _run_fullwave(ctx, mp, name, label):
    import fullwave_cases as fc
    import test_gpu_fullwave as tf
    got = fc.run_device(ctx, name)
    tf.check_gate(got, fc.reference(name))
    return "", dict(zip(("p_max", "p_min", "psq", "trace"), got))


def _run_eikonal(ctx, mp, name, label):
    import eikonal_cases as ec
    import test_gpu_eikonal as te
    got = ec.run_device(ctx, name)
    te.check_gate(got, name)
    return "", {"T": got[0], "sweeps": np.array([got[1]]), "samples": got[2]}


_RUNNERS = {"lattice": lambda ctx, mp, arg, label: _run_lattice(ctx, mp, _lm().CASES[arg], label), "general": _run_general, "hetero": _run_hetero,
            "steer": _run_steer, "steer_medium": _run_steer_medium, "pulsed_medium": _run_pulsed_medium, "thermal": _run_thermal, "fullwave": _run_fullwave, "eikonal": _run_eikonal}


def run(ctx, mp, name, label=None, bare=False):
    """One probe or extra run on ``ctx`` -> (variant string, dict of arrays); raises where the run misses the gate of the module it comes from.
    ``bare``: without resetting the settings first -- for the probes whose imported runner sets what it needs itself (OWN_SETTINGS)."""
    label = label or name
    neutral(ctx, mp, settings=not bare)
    if name in _LATE_RUNNERS:
        return _LATE_RUNNERS[name](ctx, mp, label)
    if name in lattice_cases():
        return _run_lattice(ctx, mp, lattice_cases()[name], label)
    if name in GENERAL_PROBES:
        return _run_general(ctx, mp, GENERAL_PROBES[name], label)
    if name == "cw_gen_absorb":
        return _run_general(ctx, mp, "2a-default-jittered", label, absorb=_lm().ABSORB)
    if name in HETERO_PROBES:
        return _run_hetero(ctx, mp, HETERO_PROBES[name], label)
    if name in PULSED_PROBES:
        return _run_pulsed(ctx, mp, PULSED_PROBES[name], label)
    if name in STEER_PROBES:
        return _run_steer(ctx, mp, STEER_PROBES[name], label)
    if name in STEER_MEDIUM_PROBES:
        return _run_steer_medium(ctx, mp, STEER_MEDIUM_PROBES[name], label)
    if name in PULSED_MEDIUM_PROBES:
        return _run_pulsed_medium(ctx, mp, PULSED_MEDIUM_PROBES[name], label)
    if name in BF_PROBES:
        return _run_bf(ctx, mp, BF_PROBES[name], label)
    if name in OTHER_PROBES:
        return {"thermal": _run_thermal, "fullwave": _run_fullwave, "eikonal": _run_eikonal}[FAMILY[name]](ctx, mp, OTHER_PROBES[name], label)
    kind, arg = EXTRA_RUNS[name]
    return _RUNNERS[kind](ctx, mp, arg, label)


# ---- a CW lattice probe in stages: set-up and plan, launch and fetch, the plan again -----------------------------------------------------------------
def _plan_args(case):
    from openlifu_amd import _native as nat
    lm = _lm()
    *_, xs, ys, zs = lm.geometry(case)
    outputs = lm.OUTPUTS[case["out"]]
    flags = (nat.FIELD_FP16_CORRECTION if case["fp16"] else 0) | (nat.FIELD_DIRECTIVITY if case["dirv"] else 0)
    flags |= sum({"pmag": nat.OUT_PMAG, "intensity": nat.OUT_INTENSITY, "complex": nat.OUT_COMPLEX}[o] for o in outputs)
    return ((xs[0], ys[0], zs[0]), (xs[1] - xs[0], ys[1] - ys[0], zs[1] - zs[0]), (len(xs), len(ys), len(zs)), lm.F0, lm.C, lm.RHO, lm.P0), flags, outputs


def lattice_plan(ctx, mp, name, setup=True):
    """The set-up of run_lcase (elements, steering by kernel 1 or handed in, apertures, absorption) and olx_field_plan with its arguments; with
    setup=False only the plan, on the elements and steering the context holds."""
    lm = _lm()
    case = lattice_cases()[name]
    args, flags, _ = _plan_args(case)
    if setup:
        neutral(ctx, mp)
        mp.setenv("OLX_INTENSITY_STORED", "1") if case["stored"] else None
        pos, ori, size, *_ = lm.geometry(case)
        lm.setup_ctx(ctx, pos, ori, size, lm.foci_of(case), apod=case["apod"], solve=lm._solve(case))
        dirv, _ = lm.modifiers(case)
        if dirv is not None:
            ctx.set_element_apertures(dirv[0], dirv[2])
    ctx.field_absorption(case["absorb"])
    try:
        ctx.field_plan(*args, flags=flags)
    finally:
        ctx.field_absorption(0.0)


def lattice_launch(ctx, name):
    """Launch the plan that stands and fetch what the probe fetches -> (variant, dict of arrays) under the probe's keys."""
    case = lattice_cases()[name]
    _, _, outputs = _plan_args(case)
    ctx.field_launch()
    variant = ctx.field_variant()
    return variant, _volumes([ctx.field_fetch(f, want=outputs) for f in range(len(_lm().foci_of(case)))])


# ---- settings and acts -------------------------------------------------------------------------------------------------------------------------------
def set_setting(ctx, name, on):
    """One setting "for the plans that follow" to a non-default value, or back to its default."""
    if name == "absorption":
        ctx.field_absorption(_lm().ABSORB if on else 0.0)
    elif name == "pulse":
        ctx.field_pulse(3.0, 1.6e-7, 40) if on else ctx.field_pulse(0.0, 0.0, 0)
    elif name == "response":       # (belongs to an element table: a history switches it on after a run)
        ctx.field_pulse_response(np.zeros(ctx.n_el, dtype=np.int32), [np.array([0.5, -0.25, 0.125])]) if on else ctx.field_pulse_response()
    elif name == "medium_model":
        ctx._chk(ctx._lib.olx_field_medium_model(ctx._h, 1 if on else 0))
    elif name == "layering":
        ctx._chk(ctx._lib.olx_field_medium_layering(ctx._h, 3 if on else 1))
    else:
        raise KeyError(name)


def _grid_of_plan(ctx):
    return ctx._grid_shape


def _act_upload(ctx, mp):
    n = (9, 8, 7)
    vol = np.random.default_rng(5).uniform(0.0, 1.0, (2,) + n).astype(np.float32)
    ctx.field_upload((0.0, 0.0, 0.0), (1e-3,) * 3, n, vol, vol * vol)


def _act_hetero_on_plan(ctx, mp):
    """A medium on the plan that stands (kernel 2h or 2m takes it over), launched."""
    n = _grid_of_plan(ctx)
    cvol = np.full(n, 1500.0, dtype=np.float32)
    cvol[:, :, n[2] // 2: n[2] // 2 + 2] = 2400.0
    cvol[: n[0] // 2, :, n[2] // 2] = 2000.0
    ctx.field_set_medium(cvol, None, None)
    ctx.field_launch()
    ctx.sync()


def _act_pulsed_on_elements(ctx, mp):
    """A pulsed plan with PII and p_max on the elements and steering that stand, launched; the setting back to continuous wave."""
    from openlifu_amd import _native as nat
    ctx.field_pulse(3.0, 1.6e-7, 60)
    try:
        ctx.field_plan((-4e-3, -3e-3, 6e-3), (1e-3,) * 3, (9, 7, 8), 400e3, 1500.0, 1000.0, 1e5, flags=nat.OUT_PMAG | nat.OUT_INTENSITY | nat.OUT_PMAX | nat.OUT_PII)
        ctx.field_launch()
        ctx.sync()
    finally:
        ctx.field_pulse(0.0, 0.0, 0)


def _act_steer_map(ctx, mp):
    ctx.steer_map((-5e-3, -4e-3, 8e-3), (1e-3,) * 3, (11, 9, 10), 400e3, 1500.0, 1e5, apod_kind=1, p0=35.0, absorption=3.0)


def _act_steer_map_medium(ctx, mp):
    n = (11, 9, 10)
    cvol = np.full(n, 1500.0, dtype=np.float32)
    cvol[:, :, 3:5] = 2300.0
    avol = np.zeros(n, dtype=np.float32)
    avol[:, :, 3:5] = 4.0
    ctx.steer_map_medium((-5e-3, -4e-3, 8e-3), (1e-3,) * 3, n, 400e3, 1500.0, 1e5, sound_speed=cvol, attenuation=avol, comp="equalize")


def _act_eikonal(ctx, mp):
    import eikonal_cases as ec
    ec.run_device(ctx, "short_axis")


def _act_fullwave(ctx, mp):
    import fullwave_cases as fc
    fc.run_device(ctx, "short_axis")


def _act_thermal(ctx, mp):
    shape, h, medium, inten, sched, dt, steps, perf, pts = _thermal_args("water_to_the_boundary")
    import test_gpu_thermal as tt
    rho, cp, kap, att = medium
    ctx.thermal_plan((0.0, 0.0, 0.0), h, shape, rho, cp, kap, float(tt._np_m(att)), perfusion=perf)
    ctx.thermal_schedule(*sched, points=pts)
    ctx.thermal_source(inten.shape[0], inten)
    ctx.thermal_run(dt, 37.0, 0, 40)
    ctx.thermal_fetch()


def _act_absorption_and_back(ctx, mp):
    ctx.field_absorption(_lm().ABSORB)
    ctx.field_absorption(0.0)


def _act_apertures_again(ctx, mp):
    n = ctx.n_el
    ctx.set_element_apertures(np.tile([1.0, 0.0, 0.0], (n, 1)), np.full((n, 2), 2.7e-3))


def _act_field_scale(ctx, mp):
    ctx.field_scale(np.full(ctx._plan_foci, 2.5))


def _foci4():
    return np.array([[1.5e-3, -2.0e-3, 21e-3], [-2.5e-3, 1.0e-3, 17e-3], [0.5e-3, 0.5e-3, 24e-3]])


def _act_bf_solve(ctx, mp):
    ctx.bf_solve(_foci4(), 1500.0)


def _act_bf_solve_medium(ctx, mp):
    n = (12, 10, 14)
    cvol = np.full(n, 1500.0, dtype=np.float32)
    cvol[:, :, 4:6] = 2500.0
    ctx.bf_set_medium(cvol, (-12e-3, -10e-3, 1e-3), (2e-3,) * 3, n, 1500.0)
    ctx.bf_solve_medium(_foci4(), 1500.0)


def _act_set_steering_geometric(ctx, mp):
    """Delays that ARE geometric (the oracle's Direct delays of three other foci), handed in: infer_foci finds their foci."""
    from oracle import bf_oracle as bo
    lm = _lm()
    pos, ori, *_ = lm.geometry(lattice_cases()["cw_lat_e4m3"])
    st = [bo.beamform(pos * 1e-3, ori, f + [0.0, 1e-3, 2e-3], lm.C) for f in _foci4()]
    ctx.set_steering(np.array([s[0] for s in st]), np.array([s[1] for s in st]))


def _act_bf_solve_matrix(ctx, mp):
    M = np.eye(4)
    M[:3, 3] = [2e-3, -1e-3, 3e-3]
    M[:3, :3] = [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]
    ctx.bf_solve(_foci4(), 1500.0, matrix=M)


def _act_expect_pii_refused(ctx, mp):
    """After a continuous-wave plan the readers of the PII and of p_max are refused for want of LIVE volumes (pii_live / pmax_live), not served the
    volumes of the pulsed plan before it.  (The host buffer holds PII_MAX_FOCI volumes of the standing grid: more than any resident pulsed plan of
    these histories, should a stale flag let the copy through.)"""
    from openlifu_amd import _native as nat
    import pytest
    with pytest.raises(nat.NativeError, match="olx_field_fetch_pii: no pulse intensity integrals"):
        ctx.pii_fetch(ctx.PII_MAX_FOCI)
    with pytest.raises(nat.NativeError, match="olx_field_fetch_pmax: no p_max volumes"):
        ctx.field_fetch_all(want=("pmax",))


ACTS = {"upload": _act_upload, "hetero_on_plan": _act_hetero_on_plan, "pulsed_on_elements": _act_pulsed_on_elements, "steer_map": _act_steer_map,
        "steer_map_medium": _act_steer_map_medium, "eikonal": _act_eikonal, "fullwave": _act_fullwave, "thermal": _act_thermal,
        "absorption_and_back": _act_absorption_and_back, "apertures_again": _act_apertures_again, "field_scale": _act_field_scale,
        "bf_solve": _act_bf_solve, "bf_solve_medium": _act_bf_solve_medium, "set_steering_geometric": _act_set_steering_geometric,
        "bf_solve_matrix": _act_bf_solve_matrix, "expect_pii_refused": _act_expect_pii_refused}


# the setting -> a probe whose imported runner sets it itself: run_lcase sets the absorption, pulsed_response_cases.run_device the pulse (and
# olx_set_elements drops a response that belongs to another table), field_set_medium the model and the layering
OWN_SETTINGS = {"absorption": "cw_lat_2g", "pulse": "pulsed_plain", "response": "pulsed_plain", "medium_model": "cw_het_2m", "layering": "cw_het_2m"}
REPLAN_TWINS = {"cw_lat_absorb": "lat_2g_lossless_twin", "lat_2g_lossless_twin": "cw_lat_absorb"}      # the same elements, steering, grid and flags


# ---- the histories -----------------------------------------------------------------------------------------------------------------------------------
def _h(couplings, steps, last):
    return dict(couplings=tuple(couplings), steps=tuple(steps), last=last)


def _build_histories():
    H = {}
    r = lambda name: ("run", name)      # noqa: E731
    # 1. buffer capacity: the same kind of problem larger, then the probe; smaller, then the probe
    H["cap_outputs_larger"] = _h([1], [r("big_lattice")], ("probe", "cw_lat_2g"))                       # d_pmag, d_bfrag, d_delays / d_apod of 128 elements
    H["cap_outputs_smaller"] = _h([1], [r("cw_gen_2b"), r("cw_lat_2e")], ("probe", "cw_lat_e4m3"))
    H["cap_tab_larger"] = _h([1], [r("big_general_400el")], ("probe", "cw_gen_2a"))                     # d_tab of 400 elements, then 64
    H["cap_elements_other_then_same"] = _h([1], [r("big_general_400el"), r("cw_gen_2c")], ("probe", "cw_gen_2a"))      # olx_set_elements: reallocating (400 -> 64), then in place (64 -> 64)
    H["cap_elements_grow"] = _h([1], [r("steer_e3"), r("cw_lat_2g")], ("probe", "cw_lat_e4m3"))         # 3 -> 64 -> 256 elements
    H["cap_foci_larger"] = _h([1], [r("many_foci_lattice")], ("probe", "cw_lat_2e"))                    # 9 foci, then 2
    H["cap_foci_smaller"] = _h([1], [r("cw_lat_2f")], ("probe", "cw_lat_2g"))                           # 1 focus, then 3
    H["cap_hetero_larger"] = _h([1], [r("big_hetero")], ("probe", "cw_het_2m"))
    H["cap_hetero_models"] = _h([1], [r("cw_het_2m")], ("probe", "cw_het_2h"))
    H["cap_pulsed_larger"] = _h([1], [r("pulsed_classes_9x9")], ("probe", "pulsed_plain"))              # 81 elements, 2 foci, 3 classes; then 16 elements bare
    H["cap_pulsed_smaller"] = _h([1], [r("pulsed_plain")], ("probe", "pulsed_classes_9x9"))
    H["cap_steer_larger"] = _h([1], [r("steer_c16")], ("probe", "steer_a8_maxangle"))
    H["cap_steer_smaller"] = _h([1], [r("steer_e3")], ("probe", "steer_a8_absorb_dir"))
    H["cap_steer_medium_larger"] = _h([1], [r("steer_medium_e100")], ("probe", "steer_medium_e3"))
    H["cap_pulsed_medium_larger"] = _h([1], [r("pulsed_medium_64el")], ("probe", "pulsed_medium_slab16"))
    H["cap_thermal_larger"] = _h([1], [r("thermal_big")], ("probe", "thermal_uploaded"))
    H["cap_eikonal_larger"] = _h([1], [r("eikonal_big")], ("probe", "eikonal_short_axis"))
    H["cap_fullwave_other"] = _h([1], [r("fullwave_other")], ("probe", "fullwave_short_axis"))
    H["cap_bf_after_256el"] = _h([1], [r("cw_lat_e4m3")], ("probe", "bf_maxangle_M"))
    # ... and across families: the buffers, tables and flags one family leaves to the next (every probe runs after another family at least once)
    H["cross_2f_after_pulsed"] = _h([1, 6], [r("pulsed_plain")], ("probe", "cw_lat_2f"))
    H["cross_lat_absorb_after_hetero"] = _h([1, 6], [r("cw_het_2m")], ("probe", "cw_lat_absorb"))
    H["cross_gen_absorb_after_directivity"] = _h([1], [r("cw_lat_dir"), r("cw_gen_2b")], ("probe", "cw_gen_absorb"))
    H["cross_2b_after_lattice"] = _h([1, 2], [r("cw_lat_2g")], ("probe", "cw_gen_2b"))
    H["cross_2c_after_2f"] = _h([1, 2], [r("cw_lat_2f")], ("probe", "cw_gen_2c"))
    H["cross_2h_after_pulsed"] = _h([1, 6], [r("pulsed_classes_9x9")], ("probe", "cw_het_2h"))
    H["cross_steer_after_directivity"] = _h([1], [r("cw_lat_dir")], ("probe", "steer_a8_absorb_dir"))
    H["cross_steer_after_2a"] = _h([1], [r("cw_gen_2a")], ("probe", "steer_a8_maxangle"))
    H["cross_thermal_after_cw_and_fullwave"] = _h([1], [r("cw_lat_2g"), r("fullwave_short_axis")], ("probe", "thermal_uploaded"))
    H["cross_eikonal_after_fullwave_and_cw"] = _h([1], [r("fullwave_short_axis"), r("cw_gen_2a")], ("probe", "eikonal_short_axis"))
    H["cross_fullwave_after_eikonal_and_thermal"] = _h([1], [r("eikonal_short_axis"), r("thermal_uploaded")], ("probe", "fullwave_short_axis"))
    H["cross_classes_9x9_after_lattice_256el"] = _h([1, 6], [r("cw_lat_e4m3")], ("probe", "pulsed_classes_9x9"))
    H["cross_steer_medium_after_steer_and_hetero"] = _h([1], [r("steer_a8_maxangle"), r("cw_het_2h")], ("probe", "steer_medium_e3"))
    H["cross_pulsed_medium_after_hetero_and_pulsed"] = _h([1, 6], [r("cw_het_2m"), r("pulsed_ring30")], ("probe", "pulsed_medium_slab16"))
    H["cross_pulsed_after_pulsed_medium"] = _h([1], [r("pulsed_medium_slab16")], ("probe", "pulsed_plain"))
    H["cross_bf_medium_after_cw"] = _h([1], [r("cw_gen_2a")], ("probe", "bf_solve_medium"))
    H["cross_bf_medium_after_compensated"] = _h([1], [r("bf_compensated_quantize"), r("cw_lat_2g")], ("probe", "bf_solve_medium"))
    H["cross_bf_compensated_after_bf_medium"] = _h([1], [r("bf_solve_medium"), r("steer_medium_e3")], ("probe", "bf_compensated_quantize"))
    H["cross_thermal_resident_after_uploaded_source"] = _h([1, 6], [r("thermal_uploaded"), r("pulsed_plain")], ("probe", "thermal_resident"))
    H["cross_thermal_uploaded_after_resident_source"] = _h([1], [r("thermal_resident")], ("probe", "thermal_uploaded"))
    H["cross_lockin_after_fullwave_and_cw"] = _h([1], [r("fullwave_short_axis"), r("cw_gen_2a")], ("probe", "fullwave_lockin"))
    H["cross_fullwave_after_lockin"] = _h([1], [r("fullwave_lockin")], ("probe", "fullwave_short_axis"))
    H["cross_aperture_after_lockin_and_steer"] = _h([1], [r("fullwave_lockin"), r("steer_a8_maxangle")], ("probe", "fullwave_aperture"))
    H["cross_lockin_after_aperture"] = _h([1], [r("fullwave_aperture")], ("probe", "fullwave_lockin"))
    H["cross_uploaded_after_cw"] = _h([1, 6], [r("cw_lat_2g")], ("probe", "uploaded_analyze"))
    H["cross_uploaded_after_pulsed"] = _h([1], [r("pulsed_ring30")], ("probe", "uploaded_analyze"))
    H["cross_cw_after_uploaded"] = _h([1], [r("uploaded_analyze")], ("probe", "cw_lat_2g"))
    H["cross_bf_piecewise_after_cw"] = _h([1], [r("cw_gen_2a")], ("probe", "bf_piecewise_M"))
    # 2. upload caches (upload_if_changed: up_perm, up_colinfo, up_slot, up_jobs, up_blocks)
    H["cache_other_partitions"] = _h([2], [r("cw_lat_2g"), r("lat_2g_xfold"), r("lat_2g_pitch32")], ("probe", "cw_lat_2g"))
    H["cache_2b_between"] = _h([2], [r("cw_lat_2g"), r("shared_2b_64el")], ("probe", "cw_lat_2g"))      # kernel 2b shares d_perm / up_perm
    H["cache_larger_N_between"] = _h([2], [r("cw_lat_2g"), r("big_lattice_240el")], ("probe", "cw_lat_2g"))     # the d_perm.capacity() < 4 n rule
    H["cache_new_target_and_pattern"] = _h([2], [r("lat_2g_other_target"), r("cw_lat_2e")], ("probe", "cw_lat_2g"))   # records reused, then rebuilt
    H["cache_2f_between"] = _h([2], [r("cw_lat_e4m3"), r("cw_lat_2f")], ("probe", "cw_lat_e4m3"))       # the same 256 elements: d_slot, d_cell, d_afrag
    # 3. the `same` shortcut of olx_field_plan: the probe, something else, then the identical plan again on the elements and steering that stand
    for act in ("upload", "hetero_on_plan", "pulsed_on_elements", "steer_map", "eikonal", "fullwave", "thermal", "absorption_and_back", "apertures_again"):
        H[f"same_after_{act}"] = _h([3], [r("cw_lat_2g"), ("act", act)], ("replan", "cw_lat_2g"))
    # ... and the plan that differs from the one that stands in the absorption alone: the shortcut must not take it (REPLAN_TWINS)
    H["same_but_absorption_on"] = _h([3], [r("lat_2g_lossless_twin")], ("replan", "cw_lat_absorb"))
    H["same_but_absorption_off"] = _h([3], [r("cw_lat_absorb")], ("replan", "lat_2g_lossless_twin"))
    H["same_after_hetero_2f"] = _h([3], [r("cw_lat_2f"), ("act", "hetero_on_plan")], ("replan", "cw_lat_2f"))
    # 4. settings "for the plans that follow", left set by the step before / properly cleared
    targets = {"absorption": "cw_gen_2a", "pulse": "cw_lat_2g", "response": "pulsed_plain", "medium_model": "cw_het_2m", "layering": "cw_het_2m"}
    for s, probe in targets.items():
        H[f"setting_{s}_left_set"] = _h([4], [r("cw_lat_2e"), ("set", s, True)], ("probe", probe))
        H[f"setting_{s}_cleared"] = _h([4], [r("cw_lat_2e"), ("set", s, True), ("set", s, False)], ("probe", probe))
    # ... and left set before a probe whose imported runner sets that setting ITSELF, run without the reset (OWN_SETTINGS): here the probe's own
    # set-up, not neutral(), has to override what the step before left
    for s, probe in OWN_SETTINGS.items():
        H[f"setting_{s}_left_set_own_setup"] = dict(_h([4], [r("cw_lat_2e"), ("set", s, True)], ("probe", probe)), bare=True)
    H["setting_layering_left_set_cw"] = _h([4], [r("cw_het_2h")], ("probe", "cw_lat_2e"))              # (the 2h probe itself leaves 3 planes per layer and the sampled model set)
    H["setting_absorption_after_absorbed_plan"] = _h([4], [r("cw_lat_absorb"), r("cw_gen_absorb")], ("probe", "cw_lat_dir"))
    # 5. focus knowledge (h_foci, foci_version, infer_foci): the probe whose variant reads the foci after each step of the chain
    chain = [("act", "bf_solve"), ("act", "bf_solve_medium"), ("act", "set_steering_geometric"), ("act", "bf_solve_matrix")]
    for q in range(1, 5):
        H[f"foci_after_{chain[q - 1][1]}"] = _h([5], [r("cw_lat_e4m3")] + chain[:q], ("probe", "cw_lat_e4m3"))
    H["foci_replan_after_matrix_solve"] = _h([5], [r("cw_lat_e4m3"), ("act", "bf_solve_matrix"), r("cw_lat_2f")], ("probe", "cw_lat_e4m3"))
    # 6. derived versus stored intensity
    H["intensity_after_hetero"] = _h([6], [r("cw_het_2h")], ("probe", "cw_lat_2g"))                     # stored (heterogeneous), then derived
    H["intensity_after_pulsed"] = _h([6], [r("pulsed_ring30")], ("probe", "cw_lat_dir"))
    H["intensity_scale_then_relaunch"] = _h([6], [r("cw_lat_2g"), ("act", "field_scale")], ("relaunch", "cw_lat_2g"))
    H["intensity_stored_pin_before"] = _h([6], [r("lat_2g_stored")], ("probe", "cw_lat_2g"))
    H["intensity_stored_pin_after"] = _h([6], [r("cw_lat_2g")], ("probe", "lat_2g_stored"))
    # 7. PII and p_max residency
    H["pii_cw_between"] = _h([7], [r("pulsed_plain"), r("cw_lat_2g"), ("act", "expect_pii_refused")], ("probe", "pulsed_plain"))
    H["pii_other_grid_between"] = _h([7], [r("pulsed_ring30"), r("cw_gen_2c"), ("act", "expect_pii_refused"), r("pulsed_classes_9x9")], ("probe", "pulsed_ring30"))
    # 8. other engines between plan and launch
    for act in ("steer_map", "steer_map_medium", "eikonal", "fullwave", "thermal"):
        H[f"between_plan_and_launch_{act}"] = _h([8], [("plan", "cw_lat_2g"), ("act", act)], ("launch", "cw_lat_2g"))
    H["between_plan_and_launch_all_2f"] = _h([8], [("plan", "cw_lat_2f"), ("act", "steer_map_medium"), ("act", "eikonal"), ("act", "thermal")], ("launch", "cw_lat_2f"))
    return H


HISTORIES = _build_histories()


def run_history(ctx, mp, hid):
    """Every step of history ``hid`` on ``ctx`` -> (probe name, variant, dict of arrays) of its last step."""
    h = HISTORIES[hid]
    for q, step in enumerate(h["steps"]):
        if step[0] == "run":
            run(ctx, mp, step[1], label=f"{hid}#{q}:{step[1]}")
        elif step[0] == "set":
            set_setting(ctx, step[1], step[2])
        elif step[0] == "act":
            ACTS[step[1]](ctx, mp)
        elif step[0] == "plan":
            lattice_plan(ctx, mp, step[1])
        else:
            raise KeyError(step)
    kind, name = h["last"]
    if kind == "probe":
        return (name,) + run(ctx, mp, name, label=f"{hid}:{name}", bare=h.get("bare", False))
    if kind == "replan":
        lattice_plan(ctx, mp, name, setup=False)
    return (name,) + lattice_launch(ctx, name)
