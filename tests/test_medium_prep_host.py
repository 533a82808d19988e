"""The host preparation of medium volumes behind kernels 1m, 1a, 2h / 2m, 2ph and 4h (openlifu-python_amd/csrc/olx_medium.cpp: the grid and
volume checks, the non-trivial-plane rule, the element plane bounds, the 2 x 2 edge-clamped stencil of planes and of layers, the layering, the
one-line (kappa) detection, the compact per-plane columns, the impedance volume, the attenuation factors) has no HIP in it.  Here it is compiled
by plain g++ with AddressSanitizer + UndefinedBehaviorSanitizer together with tools/medium_check.cpp and run WITHOUT a GPU: every output is
compared bit for bit with a per-voxel restatement inside the checker, over the fixed edge cases (volume checks with NaN, +-inf, 0 and negative
values at the first, middle and last voxel, kernel 2ph's interleaved priority, the grid rules, a sound speed equal to c_ref only as a float or
only after the conversion, attenuation -0.0f, G = 3 over 7 planes + gap + 1, the one-line cases) and seeded random two- to four-material volumes on
grids from 1 x 1 x 1 to 12 x 11 x 14 (nx = 1, ny = 1, nz = 1; no plane, every plane; null sound speed, null attenuation, both null; elements on a
plane's z, below all planes and above all)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openlifu-python_amd", "csrc")
OUT = os.path.join(ROOT, "oracle", "_build")
SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror"]


@pytest.fixture(scope="module")
def checker_object():
    """tools/medium_check.cpp compiled once: it includes only the unit's header, so the same object links with the unit and with every mutation of it."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not installed")
    os.makedirs(OUT, exist_ok=True)
    obj = os.path.join(OUT, "medium_check.o")
    subprocess.check_call(["g++"] + SAN + ["-c", os.path.join(ROOT, "tools", "medium_check.cpp"), "-o", obj])
    return obj


def test_medium_preparation_under_sanitizers(checker_object):
    exe = os.path.join(OUT, "medium_check")
    subprocess.check_call(["g++"] + SAN + [checker_object, os.path.join(CSRC, "olx_medium.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for seed, cases in ((147, 300), (2026, 108)):
        r = subprocess.run([exe, str(cases), str(seed)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        assert " cases, 0 mismatches" in r.stdout, r.stdout
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]


def test_the_checker_has_teeth(tmp_path, checker_object):
    """A plane rule that only sees faster voxels, an element bound that is no longer strict, a stencil without its edge clamp and a layer sum in
    float are caught, each by a FAIL line that names the rule.  (The unclamped stencil reads past its array: the mutated unit keeps AddressSanitizer
    but lets it go on after the report, so that the checker's own comparison is what fails.)"""
    src = open(os.path.join(CSRC, "olx_medium.cpp")).read().replace('"olx_medium.h"', f'"{CSRC}/olx_medium.h"')
    mutations = {
        "plane_rule_greater": ("(double)sound_speed[ij * nz + k] != c_ref", "(double)sound_speed[ij * nz + k] > c_ref", "FAIL plane rule"),
        "bound_not_strict": ("!(oz + kf * hz > ez[e])", "!(oz + kf * hz >= ez[e])", "FAIL element bounds"),
        "no_clamp": ("const int i1 = std::min(i + 1, nx - 1),", "const int i1 = i + 1,", "FAIL stencil gather"),
        "float_layer_sum": ("double s = 0.0, a = 0.0;", "float s = 0.f, a = 0.f;", "FAIL layer sum"),
    }
    for name, (old, new, expect) in mutations.items():
        assert src.count(old) == 1, name
        mutant = tmp_path / (name + ".cpp")
        mutant.write_text(src.replace(old, new))
        exe = str(tmp_path / name)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fsanitize-recover=address", checker_object, str(mutant), "-o", exe])
        r = subprocess.run([exe, "108"], env=dict(os.environ, ASAN_OPTIONS="halt_on_error=0:detect_leaks=0"), capture_output=True, text=True, timeout=600)
        assert r.returncode != 0 and expect in r.stderr, (name, (r.stdout + r.stderr)[-2000:])
