"""Split perfectly matched layers of the full-wave model, host side (no GPU): the fp64 oracle written from DESIGN.md section 2 "full-wave
model: split layers" (tests/fullwave_pml_oracle.py) against the sponge oracle where the two must agree, the known answer of a grid much
narrower than the beam's Fresnel zone, the host helper's tables, and the refusals and the API of the option.

Known answer (water, 500 kHz, h = 0.375 mm, dt = 0.3 h / c, 12-voxel layers, pml_alpha 2, one monopole on voxel (8, 8, 3) of a
16 x 16 x 64 interior, 4 cycles, ramp 1, 340 steps), on-axis p_min at k = 20 / 40 / 60 and the whole volume with k >= 8 relative to the
on-axis peak there, against the same run on a 64 x 64 x 64 interior with split layers; measured with this oracle:
  split layers   2.98e-6  4.38e-5  2.41e-4   whole 4.19e-4
  sponge         8.40e-3  1.52e-1  2.76e-1   whole 7.10e-2
The split gates are those values rounded to two digits (3.0e-6, 4.4e-5, 2.4e-4, 4.2e-4) plus half again, the rule of
tests/test_fullwave_host.py; the sponge's loss at k = 60 is asserted to stay at least 0.2.  (A 48-wide split reference differs from
the 64-wide one by 5.0e-7 at k = 60, a 48-wide sponge reference from it by 1.2e-3: the reference is converged.)"""
import functools

import numpy as np
import pytest

import openlifu_amd as ol
from openlifu_amd.sim import fullwave as fw
import fullwave_cases as fc
import fullwave_oracle as fo
import fullwave_pml_cases as pc
import fullwave_pml_oracle as po

SPLIT_AXIS = (3.0e-6, 4.4e-5, 2.4e-4)
SPLIT_WHOLE = 4.2e-4
SPONGE_LOSS_K60 = 0.2


def _both(k, steps, trace=None):
    args = (k["n"], k["h"], k["c"], k["rho"], k["alpha"], k["c_ref"], k["pml"], k["pml_alpha"], k["dt"], steps, k["ijk"], k["amp"], k["tau"], k["freq"],
            k["cycles"], k["ramp"])
    tr = k["trace"] if trace is None else trace
    return po.simulate(*args, trace_ijk=tr), fo.simulate(*args, trace_ijk=tr)


# ---- 1. agreement with the sponge oracle ----------------------------------------------------------------------------------------------
def test_without_layers_the_two_oracles_are_the_same_arithmetic():
    k = pc.CASES["no_layers"]
    assert k["pml"] == 0 and np.ndim(k["c"]) == 3 and np.ptp(k["c"]) > 0          # a layered medium
    split, sponge = _both(k, k["steps"])
    for key in ("p_max", "p_min", "psq", "trace"):
        assert sponge[key].max() > 0 and np.array_equal(split[key], sponge[key]), key


def test_with_layers_a_run_that_never_reaches_them_is_the_sponge_run():
    k = pc.SHORT
    n = k["n"]
    split, sponge = _both(k, k["steps"])
    # the premise: nothing has reached a layer voxel, nor the last interior voxel of an axis (whose + face lies half a voxel inside a layer)
    touched = (split["p_max"] != 0) | (split["p_min"] != 0)
    assert touched.sum() > 100
    q = k["pml"] + 1
    inner = np.zeros(n, dtype=bool); inner[q:-q, q:-q, q:-q] = True
    assert not np.any(touched & ~inner)
    for key in ("p_max", "p_min", "psq", "trace"):
        assert np.array_equal(split[key], sponge[key]), key
    # ... and a longer run does differ
    split, sponge = _both(k, 40)
    assert not np.array_equal(split["p_min"], sponge["p_min"])


# ---- 2. the known answer ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def known(interior, model):
    return po.known_answer_run(interior, model)


def test_known_answer_narrow_grid_keeps_its_on_axis_amplitude():
    wide = known((64, 64, 64), "pml")
    axis, whole = po.known_answer_deviations(known((16, 16, 64), "pml"), wide)
    print("split layers, narrow against wide:", [f"{v:.3e}" for v in axis], f"whole {whole:.3e}")
    for v, gate in zip(axis, SPLIT_AXIS):
        assert v <= 1.5 * gate
    assert whole <= 1.5 * SPLIT_WHOLE


def test_known_answer_sponge_loses_the_on_axis_amplitude():
    wide = known((64, 64, 64), "pml")
    axis, whole = po.known_answer_deviations(known((16, 16, 64), "sponge"), wide)
    print("sponge, narrow against wide split:", [f"{v:.3e}" for v in axis], f"whole {whole:.3e}")
    assert axis[2] >= SPONGE_LOSS_K60          # (the deviation |narrow - wide| / wide: what the feature is for)


# ---- 3. the host helper's tables -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,pml,alpha", [(40, 0.375e-3, 12, 2.0), (37, 0.4e-3, 6, 2.0), (13, 0.5e-3, 6, 3.5), (29, 0.5e-3, 1, 2.0), (5, 0.3e-3, 0, 2.0)])
def test_split_layer_tables(n, h, pml, alpha):
    dt, c_ref = 0.3 * h / 1500.0, 1500.0
    r, s = fw.split_layer_tables(n, h, pml, alpha, c_ref, dt)
    ro, so = po.tables(n, h, pml, alpha, c_ref, dt)
    assert r.dtype == np.float64 and r.shape == s.shape == (n,)
    assert np.all(np.abs(r - ro) <= np.spacing(ro)) and np.all(np.abs(s - so) <= np.spacing(so))
    assert np.array_equal(r, r[::-1])                                   # the low and the high side: centres mirror about (n - 1) / 2 ...
    assert np.array_equal(s[:-1], s[:-1][::-1])                         # ... the + faces about (n - 2) / 2
    assert np.all(r[pml:n - pml] == 1.0) and np.all(s[pml:n - 1 - pml] == 1.0)
    if pml:
        sig = lambda d: alpha * (c_ref / h) * (d / pml) ** 4
        half = np.exp(-sig(0.5) * dt / 2)
        assert s[n - 1 - pml] == pytest.approx(half, rel=1e-15) and s[pml - 1] == pytest.approx(half, rel=1e-15) and half < 1.0
        assert r[0] == pytest.approx(np.exp(-sig(pml) * dt / 2), rel=1e-15) and s[n - 1] == pytest.approx(np.exp(-sig(pml + 0.5) * dt / 2), rel=1e-15)
        assert np.all(np.diff(r[:pml + 1]) > 0) and np.all(r <= 1.0) and np.all(s <= 1.0)
        # the sponge's decay per step at a voxel centre is the square of r
        assert np.allclose(r * r, fw.layer_profile(n, h, pml, alpha, c_ref, dt), rtol=1e-14, atol=0)
    else:
        assert np.all(r == 1.0) and np.all(s == 1.0)


# ---- 4. refusals and API ---------------------------------------------------------------------------------------------------------------
def test_a_layer_model_that_is_not_one_of_the_two_is_refused_before_any_device_call(monkeypatch):
    monkeypatch.setattr(fw, "get_engine", lambda: (_ for _ in ()).throw(AssertionError("the device was asked for")))
    for call in (lambda: fw.run_fullwave_simulation(None, None, layer_model="split"),
                 lambda: fw.run_fullwave_steady_state(None, None, layer_model="PML"),
                 lambda: fw.steady_state_run(None, None, [1.0], [0.0], 500e3, layer_model=None),
                 lambda: ol.delay_methods.TimeReversal(layer_model="cpml")):
        with pytest.raises(ValueError, match=r"layer_model must be one of \('sponge', 'pml'\)"):
            call()
    assert fw.checked_layer_model("pml") == "pml" and fw.checked_layer_model("sponge") == "sponge"


def test_the_option_is_keyword_only_and_defaults_to_the_sponge():
    import inspect
    for fn in (fw.run_fullwave_simulation, fw.run_fullwave_steady_state, fw.steady_state_run):
        assert fn.__kwdefaults__["layer_model"] == "sponge" and "layer_model" in fn.__doc__
    for fn in (fw.run_fullwave_simulation, fw.run_fullwave_steady_state):          # the advertised signatures stay the ones the older tests pin
        assert "layer_model" not in inspect.signature(fn).parameters


def test_time_reversal_carries_the_layer_model_through_its_dict():
    TR = ol.delay_methods.TimeReversal
    m = TR(layer_model="pml")
    d = m.to_dict()
    assert d["class"] == "TimeReversal" and d["layer_model"] == "pml"
    again = ol.bf.delay_methods.DelayMethod.from_dict(d)
    assert isinstance(again, TR) and again == m and again.layer_model == "pml"
    assert ol.bf.delay_methods.DelayMethod.from_dict({"class": "TimeReversal", "layer_model": "pml"}).layer_model == "pml"
    assert TR().layer_model == "sponge" and "layer_model" not in TR().to_dict()
    assert ol.bf.delay_methods.DelayMethod.from_dict(TR().to_dict()) == TR()


def test_the_case_table_keeps_every_source_off_the_layers():
    for name, k in pc.CASES.items():
        assert not po.layer_mask(k["n"], k["pml"])[tuple(k["ijk"].T)].any(), name
        assert fo.activity_margin(k["tau"], k["cycles"] / k["freq"], k["dt"]) >= 1e-6 and 200 <= k["steps"] <= 400
    k = pc.CASES["one_interior_voxel"]
    assert k["n"][0] - 2 * k["pml"] == 1 and set(k["ijk"][:, 0]) == {6}
    assert pc.CASES["one_voxel_layers"]["pml"] == 1 and pc.CASES["no_layers"]["pml"] == 0
    # the lock-in's receivers: entries inside a layer, in a corner of three, and on both sides of the boundary
    row, vox, wt = pc.lock_table()
    kk = pc.CASES[pc.LOCK_CASE]
    lay = po.layer_mask(kk["n"], kk["pml"]).reshape(-1)[vox]
    assert lay.any() and not lay.all() and len(row) == 6
