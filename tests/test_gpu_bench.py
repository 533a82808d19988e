"""The driver's contract with bench.py (one JSON line on stdout): run as the driver runs it, in a fresh child process, with few steps and
a short CPU sample; every key the contract names must be there with the right type, the metric must be BASELINE.json's, and the numbers
must be consistent with each other (value = voxel-elements per step / time, roofline.frac = achieved / peak)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _clean_env():
    env = dict(os.environ)
    for k in ("OLX_FIELD_VARIANT", "OLX_FP8_CORRECTION", "OLX_EXP_KGRP", "OLX_LIB_PATH"):
        env.pop(k, None)
    return env


def test_bench_prints_one_json_line_with_the_contract_keys():
    env = _clean_env()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "5", "--warmup", "2", "--cpu-seconds", "1", "--no-extras", "--full"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    base = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    assert base["metric"].startswith(d["metric"]) and d["unit"] == "Mvoxel-elements/s" and d["metric"].startswith(d["unit"]), (d["metric"], d["unit"])
    assert d["n_gpus"] == 1 and d["steps"] == 5 and d["warmup"] == 2 and d["higher_is_better"] is True
    assert d["scaling"] in ("weak", "strong") and d["data"] == "synthetic" and d["vs_baseline"] is None
    assert isinstance(d["dtype"], str) and "workload" in d["config"] and "model" not in d["config"]
    assert d["value"] > 0 and d["ms_per_step"] > 0
    r = d["roofline"]
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s") and r["peak"] > 0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) <= 1e-9 * r["frac"] and 0 < r["frac"] < 1
    assert r["traffic"] is None or r["traffic"] > 0
    c = d["cpu_baseline"]
    assert c["value"] > 0 and c["cores"] >= 1 and c["kind"] in ("reference", "port") and isinstance(c["sample"], str) and c["unit"] == d["unit"]
    # value = Mvoxel-elements of one step / its time: 256 elements x 256^3 voxels x 8 foci per step on the headline workload
    per_step = 256 * 256 ** 3 * 8 / 1e6
    assert abs(d["value"] - per_step / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"], (d["value"], d["ms_per_step"])


def test_plain_bench_times_the_headline_only_and_dumps_its_outputs(tmp_path):
    """Without --full the line holds the headline alone (no CPU baselines, legs, parity or counter passes), `--steps` sets the timed steps,
    and --dump-outputs writes the last timed step's |p| and intensity volumes as a float32 voxel sample within 64 MB."""
    import numpy as np
    out = tmp_path / "outputs"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--dump-outputs", str(out)],
                       cwd=ROOT, env=_clean_env(), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["steps"] == 7 and d["warmup"] == 2 and d["ms_per_step"] > 0 and d["value"] > 0 and d["higher_is_better"] is True
    assert isinstance(d["dtype"], str) and d["unit"] == "Mvoxel-elements/s"
    for k in ("cpu_baseline", "cpu_baseline_c", "parity", "legs", "scans", "kernel1", "end_to_end", "achievable", "precision_safe", "library_default"):
        assert k not in d, k
    files = {f.name: np.load(f) for f in out.iterdir()}
    assert sorted(files) == ["intensity.npy", "intensity_max.npy", "pmag.npy", "pmag_max.npy"], sorted(files)
    assert sum((out / f).stat().st_size for f in files) <= 64 << 20
    F = d["config"]["foci_per_gpu"]
    pm, it = files["pmag.npy"], files["intensity.npy"]
    assert all(a.dtype == np.float32 for a in files.values())
    assert pm.shape == it.shape and pm.shape[0] == F and 0 < pm.shape[1] < 256 ** 3 and files["pmag_max.npy"].shape == (F,)
    assert np.isfinite(pm).all() and (pm >= 0).all() and (pm.max(axis=1) <= files["pmag_max.npy"]).all() and (files["pmag_max.npy"] > 0).all()
    # the same voxels in both samples: intensity = 1e-4 |p|^2 / (2 rho c) in water (include/olx.h)
    big = pm > 1e-3 * pm.max()
    assert np.allclose(it[big], 1e-4 * pm[big].astype(np.float64) ** 2 / (2 * 1000.0 * 1500.0), rtol=1e-4)
