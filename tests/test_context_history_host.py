"""The tables of the context-history matrix (tests/context_history_cases.py), checked without a GPU: every coupling and every setting is named by a
history, every probe runs after another family, the size caps hold, and the lattice rows made for the probes reach the variant they name in the real
planning code and have a finite, sensitive reference.  (The rows imported from the other matrices are checked by those matrices' own host tests.)"""
import numpy as np

import context_history_cases as hc


def _runs(h):
    return [s[1] for s in h["steps"] if s[0] in ("run", "plan")]


def _family(name):
    if name in hc.FAMILY:
        return hc.FAMILY[name]
    if name in hc.lattice_cases():
        return "cw_lattice"
    return {"lattice": "cw_lattice", "general": "cw_general", "hetero": "cw_hetero"}.get(hc.EXTRA_RUNS[name][0], hc.EXTRA_RUNS[name][0])


def test_every_step_names_something_that_exists():
    for hid, h in hc.HISTORIES.items():
        assert 1 <= len(h["steps"]) + 1 <= hc.MAX_STEPS, hid
        for s in h["steps"]:
            assert s[0] in ("run", "set", "act", "plan"), (hid, s)
            if s[0] == "run":
                assert s[1] in hc.PROBES or s[1] in hc.EXTRA_RUNS or s[1] in hc.lattice_cases(), (hid, s)
            if s[0] == "set":
                assert s[1] in hc.SETTINGS and isinstance(s[2], bool), (hid, s)
            if s[0] == "act":
                assert s[1] in hc.ACTS, (hid, s)
            if s[0] == "plan":
                assert s[1] in hc.LATTICE_PROBES, (hid, s)
        kind, name = h["last"]
        assert kind in ("probe", "replan", "launch", "relaunch"), hid
        assert name in hc.PROBES or name in hc.lattice_cases(), (hid, name)
        if kind != "probe":
            assert name in hc.lattice_cases(), hid
        if kind == "launch":        # the plan that is launched is the last thing planned: a ("plan", name) step, with acts only after it
            q = max(i for i, s in enumerate(h["steps"]) if s[0] == "plan")
            assert h["steps"][q][1] == name and all(s[0] == "act" for s in h["steps"][q + 1:]), hid
        if kind in ("replan", "relaunch"):      # the elements and the steering that stand are the probe's: its run, then acts only
            q = max(i for i, s in enumerate(h["steps"]) if s[0] == "run")
            assert h["steps"][q][1] in (name, hc.REPLAN_TWINS.get(name)) and all(s[0] == "act" for s in h["steps"][q + 1:]), hid
    lm, cases = hc._lm(), hc.lattice_cases()
    for a, b in hc.REPLAN_TWINS.items():        # twins: one plan in every argument but the absorption
        assert {k: v for k, v in cases[a].items() if k not in ("absorb", "frag", "want")} == {k: v for k, v in cases[b].items() if k not in ("absorb", "frag", "want")}
        assert (cases[a]["absorb"] > 0) != (cases[b]["absorb"] > 0) and lm._solve(cases[a])


def test_every_coupling_has_a_history():
    seen = {c for h in hc.HISTORIES.values() for c in h["couplings"]}
    assert seen == set(hc.COUPLINGS), seen
    by = {c: [hid for hid, h in hc.HISTORIES.items() if c in h["couplings"]] for c in hc.COUPLINGS}
    # 1: outputs, tables, steering, pulsed tables, steering-map volumes, thermal, full-wave and eikonal buffers; another element count; another focus count
    last_families = {_family(hc.HISTORIES[hid]["last"][1]) for hid in by[1]}
    assert last_families >= {"cw_lattice", "cw_general", "cw_hetero", "pulsed", "steer", "thermal", "fullwave", "eikonal", "bf"}, last_families
    assert any("elements" in hid for hid in by[1]) and any("foci" in hid for hid in by[1])
    h = hc.HISTORIES["cap_elements_other_then_same"]        # another N (the reallocating path of olx_set_elements), then the same N (in place)
    n = [hc.probe_shape(x)[1] if x in hc.PROBES else None for x in _runs(h)] + [hc.probe_shape(h["last"][1])[1]]
    assert n[-2] == n[-1] == 64
    # 2: another partition, kernel 2b between, a larger N between, a new target and a changed pattern
    assert {"cache_other_partitions", "cache_2b_between", "cache_larger_N_between", "cache_new_target_and_pattern"} <= set(by[2])
    assert hc.lattice_cases()["lat_2g_other_target"]["foci"] == hc.lattice_cases()["cw_lat_2g"]["foci"]
    # 3: the identical re-plan after each of the nine
    acts3 = {s[1] for hid in by[3] for s in hc.HISTORIES[hid]["steps"] if s[0] == "act"}
    assert acts3 >= {"upload", "hetero_on_plan", "pulsed_on_elements", "steer_map", "eikonal", "fullwave", "thermal", "absorption_and_back", "apertures_again"}
    assert all(hc.HISTORIES[hid]["last"][0] == "replan" for hid in by[3])
    # 5: the probe whose variant reads the foci after each step of the chain
    acts5 = [tuple(s[1] for s in hc.HISTORIES[hid]["steps"] if s[0] == "act") for hid in by[5]]
    chain = ("bf_solve", "bf_solve_medium", "set_steering_geometric", "bf_solve_matrix")
    assert all(chain[:q] in acts5 for q in range(1, 5)) and all(hc.HISTORIES[hid]["last"][1] == "cw_lat_e4m3" for hid in by[5])
    assert hc.lattice_cases()["cw_lat_e4m3"]["e4m3"]
    # 6: stored -> derived, field_scale then relaunch, the stored pin before a derived plan
    assert any(hc.HISTORIES[hid]["last"][0] == "relaunch" and ("act", "field_scale") in hc.HISTORIES[hid]["steps"] for hid in by[6])
    assert any(_family(_runs(hc.HISTORIES[hid])[-1]) in ("pulsed", "cw_hetero") and _family(hc.HISTORIES[hid]["last"][1]) in ("cw_lattice", "cw_modifier") for hid in by[6])
    assert any(_runs(hc.HISTORIES[hid]) == ["lat_2g_stored"] for hid in by[6])
    # 7: pulsed with PII -> CW on another grid (readers refused) -> the pulsed plan again
    for hid in by[7]:
        h = hc.HISTORIES[hid]
        assert _family(_runs(h)[0]) == "pulsed" and ("act", "expect_pii_refused") in h["steps"] and h["last"][1] == _runs(h)[0], hid
    # 8: the other engines between plan and launch
    acts8 = {s[1] for hid in by[8] for s in hc.HISTORIES[hid]["steps"] if s[0] == "act"}
    assert acts8 >= {"steer_map", "steer_map_medium", "eikonal", "fullwave", "thermal"} and all(hc.HISTORIES[hid]["last"][0] == "launch" for hid in by[8])


def test_every_setting_is_left_set_and_cleared():
    for s in hc.SETTINGS:
        left = [hid for hid, h in hc.HISTORIES.items() if 4 in h["couplings"] and ("set", s, True) in h["steps"] and ("set", s, False) not in h["steps"]]
        cleared = [hid for hid, h in hc.HISTORIES.items() if 4 in h["couplings"] and ("set", s, True) in h["steps"] and h["steps"][-1] == ("set", s, False)]
        assert left and cleared, (s, left, cleared)
        assert {hc.HISTORIES[hid]["last"] for hid in left} & {hc.HISTORIES[hid]["last"] for hid in cleared}, s      # the same probe either way


def test_every_probe_follows_another_family():
    for name in hc.PROBES:
        hits = [hid for hid, h in hc.HISTORIES.items() if h["last"][1] == name and any(_family(x) != _family(name) for x in _runs(h))]
        assert hits, name


def test_size_caps():
    for name in hc.PROBES:
        vox, n_el, F = hc.probe_shape(name)
        assert vox <= hc.MAX_VOXELS and n_el <= hc.MAX_ELEMENTS, (name, vox, n_el)
        assert F <= hc.MAX_FOCI or hc.CAP_EXCEPTIONS.get(name) == "foci", (name, F)
    assert set(hc.CAP_EXCEPTIONS) == {"uploaded_analyze"} and hc.probe_shape("uploaded_analyze")[2] == 8      # the one named exception: the scan matrix's dyadic-frame row
    assert len(hc.HISTORIES) >= 50


def test_the_required_probes_are_there_by_name():
    """Every probe the matrix was asked for, by name, with a runner, a family and a history that ends in it after another family."""
    assert set(hc.REQUIRED_PROBES) <= set(hc.PROBES), set(hc.REQUIRED_PROBES) - set(hc.PROBES)
    assert len(set(hc.REQUIRED_PROBES)) == 29
    families = {hc.FAMILY[n] for n in hc.REQUIRED_PROBES}
    assert families >= {"cw_lattice", "cw_general", "cw_modifier", "cw_hetero", "pulsed", "pulsed_medium", "bf", "bf_medium", "steer", "steer_medium", "thermal",
                        "fullwave", "fullwave_lockin", "fullwave_aperture", "eikonal", "uploaded"}, families
    for s, probe in hc.OWN_SETTINGS.items():       # the left-set rows that run without the reset
        h = hc.HISTORIES[f"setting_{s}_left_set_own_setup"]
        assert h["bare"] and h["steps"][-1] == ("set", s, True) and h["last"] == ("probe", probe), s
    import fullwave_aperture_cases as ac
    import fullwave_lockin_cases as lc
    import test_gpu_scan_matrix as sm
    assert hc.FULLWAVE_LOCKIN_CASE in lc.LOCK_CASES and hc.FULLWAVE_APERTURE_CASE in ac.CASES
    assert hc.uploaded_row() in sm.rows("analyze") or hc.uploaded_row()["entry"] == "analyze"


def test_the_probes_come_from_the_tables_that_have_oracles():
    import eikonal_cases as ec
    import fullwave_cases as fc
    import pulsed_response_cases as pc
    import pulsed_medium_cases as pmc
    import test_gpu_steering as ts
    import test_gpu_steering_medium as tsm
    import test_gpu_thermal as tt
    fm, hm, lm = hc._fm(), hc._hm(), hc._lm()
    assert all(v in fm.CASES for v in hc.GENERAL_PROBES.values()) and all(v in hm.CASES for v in hc.HETERO_PROBES.values())
    assert {fm.CASES[v]["want"].split("<")[0] for v in hc.GENERAL_PROBES.values()} == {"field_accum_k", "field_shared_k", "field_mfma_k"}
    assert {hm.CASES[v]["want"].split("<")[0] for v in hc.HETERO_PROBES.values()} == {"field_hetero_k", "field_hmarch_k"}
    assert all(v[0] in pc.CASES for v in hc.PULSED_PROBES.values()) and all(v in ts.CASES for v in hc.STEER_PROBES.values())
    assert pc.CASES["unit_tap"]["n"] == (13, 11, 15)
    assert hc.OTHER_PROBES["thermal_uploaded"] in tt.CASES and hc.OTHER_PROBES["fullwave_short_axis"] in fc.CASES and hc.OTHER_PROBES["eikonal_short_axis"] in ec.CASES
    assert all(v in tsm.CASES for v in hc.STEER_MEDIUM_PROBES.values()) and all(v in pmc.CASES for v in hc.PULSED_MEDIUM_PROBES.values())
    for kind, arg in hc.EXTRA_RUNS.values():
        table = {"steer_medium": tsm.CASES, "pulsed_medium": pmc.CASES, "lattice": lm.CASES, "general": fm.CASES, "hetero": hm.CASES, "steer": ts.CASES, "thermal": tt.CASES, "fullwave": fc.CASES, "eikonal": ec.CASES}[kind]
        assert arg in table, (kind, arg)


def test_the_new_lattice_rows_reach_their_variant_and_have_a_reference():
    """The rows made for the probes with test_gpu_lattice_matrix's generator: the real decision (olxplan::decide_variant) names the variant and the
    fragments each row waits for and agrees with the restated rule; the reference of focus 0 is finite with a positive maximum, a silent element row
    moves it by more than ten gates of every output compared, and the size stays under that module's cap."""
    lm = hc._lm()
    kernels = set()
    for name, case in hc.lattice_cases().items():
        line = lm._agrees(case, name)
        assert line.split(">")[0] + ">" == case["want"], (name, line)
        for frag in case["frag"]:
            assert frag in line, (name, frag, line)
        assert "from plane" not in line and ("fp8corr" in line) == case["e4m3"], (name, line)
        assert lm.n_terms(case) <= lm.CAP, name
        kernels.add(case["want"].split("<")[0])
        pos, ori, size, xs, ys, zs = lm.geometry(case)
        delays, ap = lm.steering(case)
        dirv, absorb = lm.modifiers(case)
        kw = dict(dmin=0.5 * min(xs[1] - xs[0], ys[1] - ys[0], zs[1] - zs[0]), directivity=dirv, absorption=absorb)
        area = size[:, 0] * size[:, 1] * 1e-6
        ref = lm.co.field_on_grid(xs, ys, zs, pos * 1e-3, area, delays[0], ap[0], lm.F0, lm.C, lm.P0, **kw)
        assert np.isfinite(ref.view(np.float64)).all() and np.abs(ref).max() > 0, name
        a = ap[0].copy()
        a[np.arange(len(a)) % case["arr"][1] == case["arr"][1] - 1] = 0.0
        dist = lm._distance(case, lm.co.field_on_grid(xs, ys, zs, pos * 1e-3, area, delays[0], a, lm.F0, lm.C, lm.P0, **kw), ref)
        for o in lm.OUTPUTS[case["out"]]:
            assert dist[o] > 10 * lm.GATES[o], (name, o, dist[o])
    assert kernels == {"field_cosetp_k", "field_coset_k", "field_toep_k"}
    assert hc.lattice_cases()["cw_lat_2g"]["arr"] == (8, 8) and hc.lattice_cases()["cw_lat_2g"]["pitch"] == (3, 3) and hc.lattice_cases()["cw_lat_2f"]["arr"][0] == 16
