"""Does a result depend on what its context did before?  openlifu_amd.engine.get_engine() keeps ONE olx_ctx for the life of the process, while almost
every other GPU test starts from a fresh one.  Here every probe of tests/context_history_cases.py -- one small complete operation per kernel family,
taken from the matrices that have fp64 oracles and run through their own runners and gates -- is run

  (a, b) on a fresh context, twice: it passes its module's gate, and the second fresh context gives the same bits and the same variant string;
  (c)    at the end of every history of the table (grow-only buffers, upload caches, the re-plan shortcut, settings left set, focus knowledge,
         derived / stored intensity, PII residency, other engines between plan and launch): the same bits and variant string again;
  (d)    with a setting "for the plans that follow" (include/olx.h) changed BETWEEN plan and launch: the plan carries what it was planned with;
         olx_set_elements / olx_set_element_apertures there make olx_field_launch refuse (OLX_ESTATE);
  (e)    through the Python API on the engine's own context: calc_solution, a pulsed calc_solution, a steering map, a thermal run, then the first
         calc_solution again;
  (f)    the capacity and cache histories once more in a child process against the debug library, whose olx_sync reports every index a kernel
         formed outside its extent.

Comparisons are np.array_equal on the bit patterns.  The only outputs summed with fp64 atomics are the moments of the uploaded-result probe's analysis
(returned under the "atomic:" prefix) and the centroids of (e): those are compared at rtol = atol = 1e-12, the run-to-run bound tests/test_gpu_pulsed.py
uses for them.  No other tolerance is used in (b) - (e)."""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

import context_history_cases as hc
from openlifu_amd import _native as nat

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "openlifu-python_amd", "lib")
LAST_NAMES = sorted({h["last"][1] for h in hc.HISTORIES.values()} | set(hc.PROBES), key=lambda n: (n not in hc.PROBES, n))
_FRESH = {}
# The children's limits: the measured duration of the whole child (interpreter start, imports and its check that the libraries are built included)
# plus 3 x that as margin.  Measured on an MI355X with this commit's libraries built; the parent commit has neither test, and its library runs the
# same kernels for the same histories (all of them come out equal there).
DEBUG_CHILD_SECONDS, DEBUG_CHILD_TIMEOUT = 5.65, 23        # (f): the histories of couplings 1 and 2 with their fresh references, debug library
ENGINE_CHILD_SECONDS, ENGINE_CHILD_TIMEOUT = 1.70, 7       # (e): five calls through the Python API


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 16: np.uint64}.get(a.dtype.itemsize, np.uint8))


def first_difference(fresh, got):
    """None where the two (variant, dict of arrays) agree bit for bit, else a description: the variant strings where they differ, and the first output
    that differs with its largest difference in units of the fresh output's maximum."""
    said = [] if fresh[0] == got[0] else [f"variant: {got[0]!r} != fresh {fresh[0]!r}"]
    if set(fresh[1]) != set(got[1]):
        return "; ".join(said + [f"outputs: {sorted(got[1])} != fresh {sorted(fresh[1])}"])
    for key in sorted(fresh[1]):
        a, b = fresh[1][key], got[1][key]
        if a.shape != b.shape or a.dtype != b.dtype:
            return "; ".join(said + [f"{key}: {b.dtype}{b.shape} != fresh {a.dtype}{a.shape}"])
        if key.startswith(hc.ATOMIC):       # summed with fp64 atomics: the run-to-run bound, not the bits
            if not np.allclose(a, b, rtol=1e-12, atol=1e-12, equal_nan=True):
                said.append(f"{key}: max |difference| = {float(np.abs(b - a).max()):.3e} (fp64 atomic sums: gate 1e-12)")
                break
            continue
        if not np.array_equal(bits(a), bits(b)):
            scale = float(np.abs(a).max()) or 1.0
            worst = float(np.abs(b.astype(np.complex128) - a.astype(np.complex128)).max()) / scale
            said.append(f"{key}: max |difference| = {worst:.3e} of the fresh maximum, {int((bits(a) != bits(b)).sum())} words differ")
            break
    return "; ".join(said) or None


def on_fresh_context(fn):
    """fn(ctx) on a context of its own, synchronised (the debug library reports its kernels' bounds checks there) and closed."""
    ctx = nat.Context(0)
    try:
        out = fn(ctx)
        ctx.sync()
        return out
    finally:
        ctx.close()


def fresh(name, mp):
    if name not in _FRESH:
        _FRESH[name] = on_fresh_context(lambda ctx: hc.run(ctx, mp, name, label=f"fresh:{name}"))
    return _FRESH[name]


# ---- (a), (b) ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LAST_NAMES)
def test_fresh_is_right_and_repeatable(name, monkeypatch):
    """The probe on a fresh context passes the gate of the module it was taken from (its runner asserts it), names a variant of its family, and a
    second fresh context gives the same bits and the same variant string."""
    first = fresh(name, monkeypatch)
    if name in hc.lattice_cases():
        assert first[0].startswith(hc.lattice_cases()[name]["want"]), first[0]
    assert first[1] and all(np.isfinite(v.astype(np.complex128)).all() for v in first[1].values()), name
    second = on_fresh_context(lambda ctx: hc.run(ctx, monkeypatch, name, label=f"fresh again:{name}"))
    diff = first_difference(first, second)
    print(f"FRESH {name} | {first[0].split('>')[0]} | {'repeatable' if diff is None else diff}")
    assert diff is None, (name, diff)


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hid", list(hc.HISTORIES))
def test_history_does_not_matter(hid, monkeypatch):
    name = hc.HISTORIES[hid]["last"][1]
    want = fresh(name, monkeypatch)
    got = on_fresh_context(lambda ctx: hc.run_history(ctx, monkeypatch, hid))
    assert got[0] == name
    diff = first_difference(want, got[1:])
    print(f"HISTORY {hid} | {name} | {'equal' if diff is None else diff}")
    assert diff is None, (hid, name, diff)


# ---- (d) ---------------------------------------------------------------------------------------------------------------------------------------------
# Read before any of these ran (olx.hip, k_accum.hip, k_pulse.hip): every buffer the second launch reads is sized by olx_field_plan /
# olx_field_set_medium or by the configure_variant call of that very launch -- d_tab holds TAB_STRIDE floats per (focus, element) whether or not the
# coordinates are split, d_tab2 is read only under the PLAN's directivity flag, the pulsed launch reads the PulseParams and response tables plan_pulse
# made (its dt "of the plan, not of a later olx_field_pulse"), the heterogeneous launch reads what olx_field_set_medium built.  A live setting could
# only select another kernel over correctly sized buffers, i.e. give wrong VALUES; none of the sequences can leave a buffer's extent.
OTHER = np.array([0.7e-3, -0.4e-3, 1.1e-3])       # the first launch steers here, off the probe's own foci


def _general_absorb(ctx, mp, change):
    fm, lm = hc._fm(), hc._lm()
    case = fm.CASES["2a-default-jittered"]
    pos, ori, size = fm.array(case["arr"])
    xs, ys, zs = fm.grid(case)
    fm.setup_ctx(ctx, pos, ori, size, fm.foci_of(case) + OTHER, apod=case["apod"])
    ctx.field_absorption(lm.ABSORB)
    ctx.field_plan((xs[0], ys[0], zs[0]), (xs[1] - xs[0], ys[1] - ys[0], zs[1] - zs[0]), (len(xs), len(ys), len(zs)), fm.F0, fm.C, fm.RHO, fm.P0,
                   flags=nat.OUT_PMAG | nat.OUT_INTENSITY)
    ctx.field_launch()
    change(ctx)
    st = [fm.bo.beamform(pos * 1e-3, ori, f, fm.C, apod=case["apod"]) for f in fm.foci_of(case)]
    ctx.set_steering(np.array([s[0] for s in st]), np.array([s[1] for s in st]))
    ctx.field_launch()
    return ctx.field_variant(), hc._volumes([ctx.field_fetch(f, want=("pmag", "intensity")) for f in range(len(st))])


def _lattice_absorb(ctx, mp, change):
    lm = hc._lm()
    case = hc.lattice_cases()["cw_lat_absorb"]
    args, flags, outputs = hc._plan_args(case)
    pos, ori, size, *_ = lm.geometry(case)
    lm.setup_ctx(ctx, pos, ori, size, lm.foci_of(case) + OTHER, apod=case["apod"], solve=True)
    ctx.field_absorption(case["absorb"])
    ctx.field_plan(*args, flags=flags)
    ctx.field_launch()
    change(ctx)
    ctx.bf_solve(lm.foci_of(case), lm.C)           # (the probe's own steering: kernel 1, uniform apodization)
    return hc.lattice_launch(ctx, "cw_lat_absorb")


def _pulsed(probe):
    def run(ctx, mp, change):
        import pulsed_response_cases as pc
        from oracle import bf_oracle as bo
        name, response = hc.PULSED_PROBES[probe]
        k = pc.case(name)
        ctx.set_elements(k.pos_m, np.tile([0.0, 0.0, 1.0], (len(k.pos_m), 1)), k.area)
        ctx.set_steering(np.array([bo.beamform(k.pos_m, np.zeros_like(k.pos_m), f + OTHER, pc.C)[0] for f in k.foci_m]), k.apod)
        ctx.field_absorption(k.absorption)
        ctx.field_pulse(k.cycles, k.dt, k.n_t)
        if response:
            ctx.field_pulse_response(k.cls, k.taps)
        ctx.field_plan((k.xs[0], k.ys[0], k.zs[0]), k.sp, k.n, pc.F0, pc.C, pc.RHO, pc.P0, flags=nat.OUT_PMAG | nat.OUT_INTENSITY | nat.OUT_PMAX | nat.OUT_PII)
        ctx.field_launch()
        change(ctx)
        ctx.set_steering(k.delays, k.apod)
        ctx.field_launch()
        out = ctx.field_fetch_all(want=("pmag", "intensity", "pmax", "pii"))
        return ctx.field_variant(), dict(out, trace=ctx.field_pulse_trace(k.trace_voxels()))
    return run


def _hetero(probe, before_medium=None):
    def run(ctx, mp, change):
        hm = hc._hm()
        case = hm.CASES[hc.HETERO_PROBES[probe]]
        hm._env(mp, case)
        pos, ori, size = hm.array(case["arr"])
        xs, ys, zs = hm.grid(case)
        cvol, avol, rvol = hm.medium(case)
        outputs = hm.fm.OUTPUTS[case["out"]]
        hm.setup_ctx(ctx, pos, ori, size, hm.fm.foci_of(case) + OTHER, apod=case["apod"])
        ctx.field_plan((xs[0], ys[0], zs[0]), (xs[1] - xs[0], ys[1] - ys[0], zs[1] - zs[0]), (len(xs), len(ys), len(zs)), hm.F0, hm.C, hm.RHO, hm.P0,
                       flags=sum({"pmag": nat.OUT_PMAG, "intensity": nat.OUT_INTENSITY, "complex": nat.OUT_COMPLEX}[o] for o in outputs))
        if before_medium is not None:
            before_medium(ctx)
        ctx.field_set_medium(cvol, avol, rvol if case["rho"] else None, planes_per_layer=case["G"], model=case["model"])
        ctx.field_launch()
        change(ctx)
        d, ap = hm.steering(hc.HETERO_PROBES[probe])
        ctx.set_steering(d, ap)
        ctx.field_launch()
        return ctx.field_variant(), hc._volumes([ctx.field_fetch(f, want=outputs) for f in range(len(d))])
    return run


def _model(value):
    return lambda ctx: ctx._chk(ctx._lib.olx_field_medium_model(ctx._h, value))


def _layering(value):
    return lambda ctx: ctx._chk(ctx._lib.olx_field_medium_layering(ctx._h, value))


ROWS = {    # setting changed between plan and launch: (the probe whose plan it is, the staged run, the change)
    "absorption_per_pair_kernel": ("cw_gen_absorb", _general_absorb, lambda ctx: ctx.field_absorption(0.0)),
    "absorption_lattice_tables": ("cw_lat_absorb", _lattice_absorb, lambda ctx: ctx.field_absorption(0.0)),
    "absorption_raised_lattice_tables": ("cw_lat_absorb", _lattice_absorb, lambda ctx: ctx.field_absorption(95.0)),
    "pulse_back_to_cw": ("pulsed_plain", _pulsed("pulsed_plain"), lambda ctx: ctx.field_pulse(0.0, 0.0, 0)),
    "pulse_other_time_axis": ("pulsed_ring30", _pulsed("pulsed_ring30"), lambda ctx: ctx.field_pulse(7.0, 3.1e-7, 23)),
    "response_cleared": ("pulsed_ring30", _pulsed("pulsed_ring30"), lambda ctx: ctx.field_pulse_response()),
    "response_replaced": ("pulsed_classes_9x9", _pulsed("pulsed_classes_9x9"), lambda ctx: ctx.field_pulse_response(np.zeros(81, dtype=np.int32), [np.array([1.0, 0.5])])),
    "response_set_on_a_plain_plan": ("pulsed_plain", _pulsed("pulsed_plain"), lambda ctx: ctx.field_pulse_response(np.zeros(16, dtype=np.int32), [np.array([1.0, 0.5])])),
    "medium_model_sampled_to_marched": ("cw_het_2h", _hetero("cw_het_2h"), _model(2)),
    "medium_model_auto_to_sampled": ("cw_het_2m", _hetero("cw_het_2m"), _model(1)),
    "layering_3_to_1": ("cw_het_2h", _hetero("cw_het_2h"), _layering(1)),
    "absorption_raised_between_plan_and_medium": ("cw_het_2m", _hetero("cw_het_2m", before_medium=lambda ctx: ctx.field_absorption(40.0)), lambda ctx: None),
    "layering_1_to_4": ("cw_het_2m", _hetero("cw_het_2m"), _layering(4)),
}


@pytest.mark.parametrize("row", list(ROWS))
def test_a_plan_carries_the_settings_it_was_planned_with(row, monkeypatch):
    """plan under setting S -> launch -> change the setting -> the probe's own steering -> launch without re-planning: bit for bit (and in the variant
    string) the fresh probe, i.e. a fresh context that planned under S with that steering -- which passed the oracle gate computed with S."""
    probe, staged, change = ROWS[row]
    want = fresh(probe, monkeypatch)

    def go(ctx):
        hc.neutral(ctx, monkeypatch)
        return staged(ctx, monkeypatch, change)
    got = on_fresh_context(go)
    diff = first_difference(want, got)
    print(f"BETWEEN {row} | {probe} | {'equal' if diff is None else diff}")
    assert diff is None, (row, diff)


def test_a_medium_is_refused_on_a_plan_made_under_an_absorption_whatever_the_setting_says_now(monkeypatch):
    """olx_field_set_medium asks the PLAN: made under an absorption it refuses the medium (OLX_EINVAL) even after olx_field_absorption(0); the
    opposite order -- a lossless plan, the setting raised since -- takes the medium (row absorption_raised_between_plan_and_medium)."""
    def go(ctx):
        hc.neutral(ctx, monkeypatch)
        hc.lattice_plan(ctx, monkeypatch, "cw_lat_absorb")          # (plans under 40 Np/m and sets the setting back to 0)
        with pytest.raises(ValueError, match="exclude each other"):
            ctx.field_set_medium(np.full(ctx._grid_shape, 1600.0, dtype=np.float32), None, None)
        return hc.lattice_launch(ctx, "cw_lat_absorb")              # the plan still stands and launches
    assert first_difference(fresh("cw_lat_absorb", monkeypatch), on_fresh_context(go)) is None


@pytest.mark.parametrize("what", ["elements", "apertures"])
def test_a_new_element_table_between_plan_and_launch_is_refused(what, monkeypatch):
    lm = hc._lm()
    case = hc.lattice_cases()["cw_lat_dir"]

    def go(ctx):
        hc.lattice_plan(ctx, monkeypatch, "cw_lat_dir")
        before = hc.lattice_launch(ctx, "cw_lat_dir")
        pos, ori, size, *_ = lm.geometry(case)
        dirv, _ = lm.modifiers(case)
        if what == "elements":
            ctx.set_elements(pos * 1e-3, lm.bo.element_rotations(ori)[:, :, 2], size[:, 0] * size[:, 1] * 1e-6)      # the very same table
        else:
            ctx.set_element_apertures(dirv[0], dirv[2])
        with pytest.raises(nat.NativeError, match=r"\[olx -2\] olx_field_launch: call olx_field_plan first"):
            ctx.field_launch()          # (refused at the head of olx_field_launch: nothing is packed or enqueued)
        # nothing was launched and nothing stands: the resident volumes belong to the plan the new table ended, and their readers say so
        with pytest.raises(nat.NativeError, match=r"\[olx -2\] olx_field_fetch: nothing planned"):
            ctx.field_fetch(0, want=("pmag",))
        assert ctx.field_variant() == ""                 # (no plan stands, so none is named)
        return before
    assert first_difference(fresh("cw_lat_dir", monkeypatch), on_fresh_context(go)) is None


# ---- (e) ---------------------------------------------------------------------------------------------------------------------------------------------
def test_the_engines_own_context_through_the_python_api():
    """calc_solution (CW) -> calc_solution (pulsed) -> calc_steering_map -> run_thermal_simulation -> the first calc_solution again, all on the one
    context the engine keeps: the volumes of the last call are the first's bit for bit, the analysis equal (its centroids, fp64 atomic sums, to 1e-12).
    In a child process with an engine of its own, so that the engine of the process that runs the suite meets the later modules as it always did."""
    if os.environ.get("OLX_HISTORY_ENGINE_CHILD") != "1":
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", "engines_own_context", "-p", "no:cacheprovider"],
                           env=dict(os.environ, OLX_HISTORY_ENGINE_CHILD="1"), cwd=ROOT, capture_output=True, text=True, timeout=ENGINE_CHILD_TIMEOUT)
        tail = (r.stdout + r.stderr)[-3000:]
        assert r.returncode == 0 and "1 passed" in tail and "skipped" not in tail, tail
        return
    import openlifu_amd as ol
    from openlifu_amd.sim.thermal import run_thermal_simulation

    arr = ol.Transducer.gen_matrix_array(nx=8, ny=8, pitch=3, kerf=0.3, units="mm", sensitivity=1e5)

    def protocol(**options):
        setup = ol.SimSetup(spacing=1.0, x_extent=(-11.5, 11.5), y_extent=(-9.5, 9.5), z_extent=(5, 28), options=dict(options))
        return ol.Protocol(pulse=ol.Pulse(frequency=400e3, duration=2e-5), sequence=ol.Sequence(pulse_interval=0.1, pulse_count=3, pulse_train_interval=1.0, pulse_train_count=1),
                           focal_pattern=ol.focal_patterns.Wheel(center=True, num_spokes=2, spoke_radius=3.0, target_pressure=1e6),
                           sim_setup=setup, apod_method=ol.apod_methods.MaxAngle(max_angle=40.0))
    target = ol.Point(position=(0, 0, 20), units="mm")

    def cw():
        sol, agg, analysis = protocol().calc_solution(target, arr, simulate=True, scale=True)
        vols = {k: np.array(sol.simulation_result[k].data) for k in ("p_max", "p_min", "intensity")}
        vols.update({"agg_" + k: np.array(agg[k].data) for k in ("p_max", "p_min", "intensity")})
        vols.update(delays=np.array(sol.delays), apodizations=np.array(sol.apodizations))
        return sol, vols, analysis
    sol, first, first_analysis = cw()
    protocol(field_model="pulsed").calc_solution(target, arr, simulate=True, scale=True)
    proto = protocol()
    proto.calc_steering_map(arr)
    run_thermal_simulation(proto.sim_setup.setup_sim_scene(ol.seg.seg_methods.UniformWater()), sol)
    _, last, last_analysis = cw()
    for key in first:
        assert np.array_equal(bits(first[key]), bits(last[key])), key
    for fld in dataclasses.fields(first_analysis):
        a, b = getattr(first_analysis, fld.name), getattr(last_analysis, fld.name)
        if isinstance(a, (list, float)) and "centroid" in fld.name:
            assert np.allclose(np.asarray(a, dtype=float), np.asarray(b, dtype=float), rtol=1e-12, atol=1e-12, equal_nan=True), fld.name
        elif isinstance(a, (list, float)):
            assert np.array_equal(np.asarray(a, dtype=float), np.asarray(b, dtype=float), equal_nan=True), fld.name
        else:
            assert a == b, fld.name


# ---- (f) ---------------------------------------------------------------------------------------------------------------------------------------------
def test_capacity_and_cache_histories_stay_inside_their_extents_in_the_debug_library():
    """The histories of couplings 1 and 2 in one child process against the debug library: every context ends with olx_sync, which reports each index
    a kernel formed outside its extent -- a buffer sized for the problem before, a table of another partition."""
    env = dict(os.environ, OLX_LIB_PATH=os.path.join(LIB, "libolx_dbg.so"))
    for v in hc.ENV_PINS:
        env.pop(v, None)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", "history_does_not_matter and (cap_ or cache_ or cross_)",
                        "-p", "no:cacheprovider"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=DEBUG_CHILD_TIMEOUT)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in tail and "failed" not in tail and "error" not in tail.lower() and "skipped" not in tail, tail


