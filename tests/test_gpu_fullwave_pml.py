"""Split perfectly matched layers of the full-wave model on the MI355X: fullwave_vel_k<UNI, SPLIT> and fullwave_pres_split_k through the
C-ABI (olx_fullwave_layers) against the fp64 oracle written from the definition (tests/fullwave_pml_oracle.py) over the case table of
tests/fullwave_pml_cases.py, bit equalities device against device, the ABI's refusals, the public entry points, and the debug library.

Gate: each record's deviation from the oracle is measured as a fraction of the oracle's maximum; when the largest is at most a quarter of
the sponge's GATE = 2e-5 (tests/test_gpu_fullwave.py) that gate is used, otherwise eight times the measured value rounded up to one digit
(the rule tests/test_gpu_fullwave.py derived its own gate by).  Measured (gfx950), largest of p_max / p_min / sum p^2 / trace per case:
  uniform_water 1.54e-6 (sum p^2)   layered 7.2e-7 (sum p^2)   absorbing_only 1.05e-6 (trace)   density_only 7.1e-7 (sum p^2)
  one_voxel_layers 1.26e-6 (trace)   one_interior_voxel 3.3e-7 (trace)   element-factored sources 7.2e-7   p_max / p_min <= 1.9e-7 everywhere
The largest, 1.54e-6, is below 5e-6, so GATE = 2e-5.  The lock-in records keep the gates of tests/test_gpu_fullwave_lockin.py (measured:
volume 6.5e-6 of 5e-5, receivers inside the layers 1.36e-5 of 4e-5), TimeReversal and the steady state theirs (delays 7.3e-8 cycles of 3e-7,
receiver sums 6.1e-7, amplitude 2.7e-7).  run_fullwave_simulation, narrow against wide, on axis at k = 20 / 40 / 60: split layers 3.0e-6,
4.4e-5, 2.4e-4 (whole volume 4.2e-4), sponge 8.4e-3, 1.5e-1, 2.8e-1.

Bits: the split pressure kernel spells every rounding of an interior voxel out as the gfx950 code of fullwave_pres_k takes it with D = 1, and
the velocity update its fused multiply-add.  So without layers (pml_size = 0) the two models agree bit for bit, and so does a run that ends
before anything reaches a layer; both are tested here device against device, beside the oracles' own agreement in
tests/test_fullwave_pml_host.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import openlifu_amd as ol
from openlifu_amd import _native as nat
from openlifu_amd.sim import run_fullwave_simulation, run_fullwave_steady_state
import fullwave_cases as fc
import fullwave_lockin_cases as lc
import fullwave_lockin_oracle as lo
import fullwave_oracle as fo
import fullwave_pml_cases as pc
import fullwave_pml_oracle as po
import medium_delay_oracle as mo
import test_fullwave_pml_host as host
import test_gpu_fullwave_lockin as tl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "openlifu-python_amd", "lib")
GATE = 2e-5
GATE_VOLUME, GATE_RECEIVERS, GATE_DELAYS = tl.GATE_VOLUME, tl.GATE_RECEIVERS, tl.GATE_DELAYS
F0 = lc.F0


@pytest.fixture(scope="module")
def ctx():
    c = nat.Context(0)
    yield c
    c.close()


def check_gate(got, ref, what=""):
    dev = fc.deviations(got, ref)
    print(what, {k: f"{v:.3e}" for k, v in dev.items()})
    for key, v in dev.items():
        assert v <= GATE, (what, key, v)


# ---- 1. parity with the oracle ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", pc.PARITY)
def test_matches_oracle(ctx, name):
    k = pc.CASES[name]
    assert 200 <= k["steps"] <= 400 and k["pml"] > 0
    got = pc.run_device(ctx, name)
    ref = pc.reference(name)
    assert ref["p_max"].max() > 0 and ref["p_min"].max() > 0 and ref["psq"].max() > 0
    check_gate(got, ref, name)
    assert got[0].min() >= 0 and got[1].min() >= 0
    # the layers are exercised: the oracle's records are not 0 in the layer voxels, nor where three layers overlap
    lay = po.layer_mask(k["n"], k["pml"])
    assert ref["p_min"][lay].max() > 0 and ref["p_min"][0, 0, 0] > 0


@pytest.mark.gpu
def test_lockin_volume_and_receivers_inside_a_layer_match_the_oracle(ctx):
    rec, lock = pc.run_device_lockin(ctx)
    check_gate(rec, pc.reference(pc.LOCK_CASE), "lock-in run, records")
    dev = lc.deviations(lock, pc.lock_reference())
    print("lock-in", {k: f"{v:.3e}" for k, v in dev.items()})
    assert dev["volume"] <= GATE_VOLUME and dev["receivers"] <= GATE_RECEIVERS


@pytest.mark.gpu
def test_element_factored_sources_match_the_oracle(ctx):
    check_gate(pc.run_device_elements(ctx), pc.reference(pc.ELEM_CASE), "element-factored")


# ---- 2. bit equalities, device against device -------------------------------------------------------------------------------------------
def _same(a, b):
    for x, y in zip(a, b):
        assert (x is None and y is None) or np.array_equal(x, y)


@pytest.mark.gpu
def test_without_layers_the_two_models_give_the_same_bits(ctx):
    _same(pc.run_device(ctx, "no_layers", "pml"), pc.run_device(ctx, "no_layers", "sponge"))
    check_gate(pc.run_device(ctx, "no_layers", "pml"), fc.reference("lossless"), "no layers, against the sponge oracle")


@pytest.mark.gpu
def test_a_run_that_never_reaches_a_layer_is_the_sponge_run_bit_for_bit(ctx):
    split, sponge = pc.run_device(ctx, "short", "pml"), pc.run_device(ctx, "short", "sponge")
    assert np.count_nonzero(split[1]) > 100 and split[3].any()
    _same(split, sponge)


@pytest.mark.gpu
def test_continued_run_equals_one_shot_bit_for_bit(ctx):
    one = pc.run_device(ctx, "layered")
    _same(one, pc.run_device(ctx, "layered", split=137))
    _same(one, pc.run_device(ctx, "layered"))


@pytest.mark.gpu
def test_sponge_after_split_and_split_after_a_larger_sponge_equal_a_fresh_context(ctx):
    fresh = nat.Context(0)
    try:
        sponge_fresh = fc.run_device(fresh, "uniform_water")
    finally:
        fresh.close()
    fresh = nat.Context(0)
    try:
        split_fresh = pc.run_device(fresh, "uniform_water")
    finally:
        fresh.close()
    pc.run_device(ctx, "layered")                          # the split model, on a larger grid ...
    _same(fc.run_device(ctx, "uniform_water"), sponge_fresh)          # ... then a plan of its own returns to the sponge
    fc.run_device(ctx, "layered")                          # a larger sponge plan ...
    _same(pc.run_device(ctx, "uniform_water"), split_fresh)           # ... then the split model on a smaller one
    assert not np.array_equal(split_fresh[1], sponge_fresh[1])


# ---- 3. ABI -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_layers_call_out_of_order_and_bad_arguments():
    c = nat.Context(0)
    try:
        with pytest.raises(nat.NativeError, match="no full-wave plan"):
            c.fullwave_layers(1)
        k = pc.CASES["uniform_water"]
        plan = (k["h"], k["n"], 1500.0, 1000.0, 0.0, 1500.0, 6, 2.0, k["dt"])
        c.fullwave_plan(*plan)
        for bad in (2, -1):
            with pytest.raises(ValueError, match="model must be 0"):
                c.fullwave_layers(bad)
        with pytest.raises(ValueError, match="layer_model must be one of"):
            c.fullwave_plan(*plan, layer_model="split")
        in_layer = int(fc.lin([(16, 16, 3)], k["n"])[0])
        c.fullwave_sources([in_layer], [1.0], [0.0], F0, 3, 0, 10)          # the sponge takes it
        c.fullwave_layers(1)
        with pytest.raises(nat.NativeError, match="olx_fullwave_sources first"):          # the layers call cleared the sources
            c.fullwave_run(0, 10)
        with pytest.raises(ValueError, match="lies in a layer"):
            c.fullwave_sources([in_layer], [1.0], [0.0], F0, 3, 0, 10)
        with pytest.raises(ValueError, match="lies in a layer"):
            c.fullwave_sources_elements([in_layer], [0], [1.0], [1.0], [0.0], F0, 3, 0, 10)
        c.fullwave_sources([int(fc.lin([(16, 16, 6)], k["n"])[0])], [1.0], [0.0], F0, 3, 0, 10)          # the first interior voxel
        c.fullwave_run(0, 10)
        c.fullwave_layers(0)                                # back to the sponge: the same entry is accepted again
        c.fullwave_sources([in_layer], [1.0], [0.0], F0, 3, 0, 10)
        c.fullwave_plan(*plan, layer_model="pml")
        with pytest.raises(ValueError, match="lies in a layer"):
            c.fullwave_sources([in_layer], [1.0], [0.0], F0, 3, 0, 10)
        c.fullwave_plan(*plan)                              # every plan returns to the sponge
        c.fullwave_sources([in_layer], [1.0], [0.0], F0, 3, 0, 10)
        c.fullwave_run(0, 10)
        c.sync()
    finally:
        c.close()


# ---- 4. the public path -----------------------------------------------------------------------------------------------------------------
def _known_scene(width):
    """The known answer's grid of ``width`` x ``width`` x 64 voxels at 0.375 mm with one element on voxel (width / 2, width / 2, 3)"""
    h = po.KNOWN["h"] * 1e3
    half = width // 2
    setup = ol.SimSetup(spacing=h, x_extent=(-half * h, (half - 1) * h), y_extent=(-half * h, (half - 1) * h), z_extent=(-3 * h, 60 * h))
    params = setup.setup_sim_scene(ol.seg_methods.UniformWater())
    assert tuple(params.coords[d].size for d in ("x", "y", "z")) == (width, width, 64)
    arr = ol.Transducer.gen_matrix_array(nx=1, ny=1, pitch=0.3, kerf=0.05, units="mm", sensitivity=1e5)
    assert np.allclose(arr.element_table()[0], 0.0)
    return arr, params


def _known_run(width, model):
    K = po.KNOWN
    arr, params = _known_scene(width)
    dt = 0.3 * K["h"] / K["c"]
    out, raw = run_fullwave_simulation(arr, params, freq=K["freq"], cycles=K["cycles"], dt=dt, t_end=K["steps"] * dt, pml_size=K["pml"],
                                       pml_alpha=K["pml_alpha"], ramp_cycles=K["ramp"], layer_model=model)
    assert raw["n_steps"] == K["steps"] and raw["layer_model"] == model
    pmin = np.asarray(out["p_min"].data, dtype=np.float64)
    o = width // 2 - 8
    return pmin[o:o + 16, o:o + 16, :]


@pytest.mark.gpu
def test_run_fullwave_simulation_keeps_the_on_axis_amplitude_of_a_narrow_grid():
    wide = _known_run(64, "pml")
    axis, whole = po.known_answer_deviations(_known_run(16, "pml"), wide)
    print("run_fullwave_simulation, split layers, narrow against wide:", [f"{v:.3e}" for v in axis], f"whole {whole:.3e}")
    for v, gate in zip(axis, host.SPLIT_AXIS):
        assert v <= 1.5 * gate + GATE
    assert whole <= 1.5 * host.SPLIT_WHOLE + GATE
    axis, _ = po.known_answer_deviations(_known_run(16, "sponge"), wide)
    print("run_fullwave_simulation, sponge, narrow against wide split:", [f"{v:.3e}" for v in axis])
    assert axis[2] >= host.SPONGE_LOSS_K60


def _steady_oracle(sc, src, rec_points, axis, ramp, every=False):
    """lo.steady_receivers with the split-layer oracle -> (Z [P], full trace [steps, voxels] | None)"""
    n_steps, cycles, w0, nw = axis
    row, ijk, wt = lo.trilinear(rec_points, (0, 0, 0), sc["h"], sc["n"])
    if every:
        trace_ijk = np.stack(np.meshgrid(*[np.arange(v) for v in sc["n"]], indexing="ij"), axis=-1).reshape(-1, 3)
        col = {q: int(fc.lin(ijk[q], sc["n"])[0]) for q in range(len(ijk))}
    else:
        trace_ijk, col = ijk, {q: q for q in range(len(ijk))}
    tr = po.simulate(sc["n"], sc["h"], sc["c"], sc["rho"], sc["alpha"], lc.C0, sc["pml"], 2.0, sc["dt"], n_steps, src[0], src[1], src[2], F0, cycles, ramp,
                     trace_ijk=trace_ijk)["trace"]
    C, S = lo.receiver_sums(tr, col, row, np.arange(len(ijk)), wt, F0, sc["dt"], w0, nw)
    return C + 1j * S, (tr if every else None)


@pytest.mark.gpu
def test_time_reversal_with_split_layers_matches_the_oracle():
    arr, params, M, target, sc = tl._wedge_product_scene()
    axis = tl._product_axis(sc)
    src = fo.monopole_entries(sc["focus"][None], (0, 0, 0), sc["h"], [1.0], [0.0], sc["c"], F0, sc["dt"], sc["n"])
    Z, _ = _steady_oracle(sc, src, sc["pos"], axis, tl.RAMP)
    q = sc["pml"]
    crop = (slice(q, -q),) * 3
    ray = mo.delays(sc["pos"] - sc["shift"], (sc["focus"] - sc["shift"])[None], sc["c"][crop], -np.array([sc["half"], sc["half"], 0]) * sc["h"], (sc["h"],) * 3, lc.C0)[0]
    ref, margin, m, _ = lo.time_reversal(Z, ray, F0)
    assert margin >= 0.25
    method = ol.delay_methods.TimeReversal(frequency=F0, lockin_cycles=tl.LOCKIN, settle_cycles=tl.SETTLE, ramp_cycles=tl.RAMP, pml_size=q, layer_model="pml")
    delays, amps, info = method.solve(arr, target, params, transform=M)
    dev_z = np.abs(info["raw"][0]["receiver_sums"] - Z).max() / np.abs(Z).max()
    dev = np.abs(delays[0] - ref).max() * F0
    print(f"TimeReversal, split layers: delays {dev:.3e} cycles, receiver sums {dev_z:.3e} of the largest")
    assert dev_z <= GATE_RECEIVERS and dev <= GATE_DELAYS and np.array_equal(info["cycles"][0], m)
    assert np.array_equal(method.calc_delays(arr, target, params, transform=M), delays[0])
    sponge = ol.delay_methods.TimeReversal(frequency=F0, lockin_cycles=tl.LOCKIN, settle_cycles=tl.SETTLE, ramp_cycles=tl.RAMP, pml_size=q)
    assert not np.array_equal(sponge.calc_delays(arr, target, params, transform=M), delays[0])          # the option reaches the run


@pytest.mark.gpu
def test_steady_state_with_split_layers_matches_the_oracle():
    arr, params, M, target, sc = tl._wedge_product_scene()
    h, q = sc["h"], sc["pml"]
    pos = arr.element_table()[0] + sc["shift"]
    d = np.sqrt(((pos - sc["focus"]) ** 2).sum(axis=1))
    delays = (d.max() - d) / lc.C0 + 0.37e-7
    apod = np.ones(16); apod[5] = 0.0; apod[9] = 0.5
    rec = np.array([[0.0, 0.0, 1.5], [0.3, -0.7, 2.1]])
    out, raw = run_fullwave_steady_state(arr, params, delays, apod, freq=F0, amplitude=2.0, lockin_cycles=tl.LOCKIN, settle_cycles=tl.SETTLE,
                                         ramp_cycles=tl.RAMP, pml_size=q, receivers=rec, layer_model="pml")
    axis = tl._product_axis(sc, extra_delay=delays.max())
    assert raw["n_steps"] == axis[0] and raw["window"] == axis[2:] and raw["layer_model"] == "pml"
    A0 = apod * arr.element_table()[2] * 2.0 * 1e5 * F0 / lc.C0
    src = fo.monopole_entries(pos, (0, 0, 0), h, A0, delays, sc["c"], F0, sc["dt"], sc["n"])
    Zr, tr = _steady_oracle(sc, src, rec * 1e-3 + sc["shift"], axis, tl.RAMP, every=True)
    C, S = lo.volume_sums(tr, F0, sc["dt"], axis[2], axis[3])
    crop = (slice(q, -q),) * 3
    A, psi = lo.amplitude_phase(C.reshape(sc["n"])[crop], S.reshape(sc["n"])[crop], axis[3])
    got_A, got_psi = np.asarray(out["p_max"].data), np.asarray(out["phase"].data)
    dev_a = np.abs(got_A - A).max() / A.max()
    dev_p = np.abs(got_A * np.exp(2j * np.pi * got_psi) - A * np.exp(2j * np.pi * psi)).max() / A.max()
    dev_r = np.abs(raw["receiver_sums"] - Zr).max() / np.abs(Zr).max()
    print(f"steady state, split layers: amplitude {dev_a:.3e}, amplitude x phase {dev_p:.3e}; receiver sums {dev_r:.3e}")
    assert dev_a <= GATE_VOLUME + 2.0 ** -24 and dev_p <= GATE_VOLUME + (1 + np.pi) * 2.0 ** -24 and dev_r <= GATE_RECEIVERS


# ---- 5. the debug library ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_split_kernels_stay_inside_their_extents_in_the_debug_library():
    env = dict(os.environ, OLX_LIB_PATH=os.path.join(LIB, "libolx_dbg.so"))
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "from openlifu_amd import _native as nat\n"
            "import fullwave_cases as fc\n"
            "import fullwave_lockin_cases as lc\n"
            "import fullwave_pml_cases as pc\n"
            "ctx = nat.Context(0)\n"
            "for name in pc.PARITY:\n"
            "    dev = fc.deviations(pc.run_device(ctx, name), pc.reference(name))\n"
            "    assert max(dev.values()) <= %r, (name, dev)\n"
            "pc.run_device(ctx, 'layered', split=137)\n"
            "pc.run_device(ctx, 'no_layers')\n"
            "pc.run_device_elements(ctx)\n"
            "dev = lc.deviations(pc.run_device_lockin(ctx)[1], pc.lock_reference())\n"
            "assert dev['volume'] <= %r and dev['receivers'] <= %r, dev\n"
            "fc.run_device(ctx, 'uniform_water')\n"
            "ctx.sync()\n"
            "print('fullwave split-layer debug cases ok')\n") % (os.path.join(ROOT, "tests"), os.path.join(ROOT, "openlifu-python_amd"), GATE, GATE_VOLUME,
                                                                GATE_RECEIVERS)
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "fullwave split-layer debug cases ok" in tail, tail
