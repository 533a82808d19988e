"""The real kernel-2 planning code (openlifu-python_amd/csrc/olx_plan.cpp) behind the C interface of tools/plan_query.cpp, for the CPU sections of the
parity matrices: planq() builds and loads the library (dev=True: with -DOLX_DEV_PINS, which honours the forcing value of OLX_FP8_CORRECTION as the
developer library does), variant() returns the variant string of the real decision (olxplan::decide_variant) for a plan given as plain arrays."""
import ctypes
import functools
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAG = {"pmag": 1, "intensity": 2, "complex": 4, "directivity": 16, "fp16": 32}      # include/olx.h


@functools.lru_cache(maxsize=None)
def planq(dev=False):
    out = os.path.join(ROOT, "oracle", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libplan_query_dev.so" if dev else "libplan_query.so")
    srcs = [os.path.join(ROOT, "tools", "plan_query.cpp"), os.path.join(ROOT, "openlifu-python_amd", "csrc", "olx_plan.cpp")]
    deps = srcs + [os.path.join(ROOT, "openlifu-python_amd", "csrc", h) for h in ("olx_plan.h", "olx_params.h", "k_toep.hip.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-shared", "-fPIC"] + (["-DOLX_DEV_PINS"] if dev else []) + srcs + ["-o", so])
    lib = ctypes.CDLL(so)
    lib.olq_coset_tiles16.restype = ctypes.c_longlong
    return lib


def _d(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _i(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def variant(pos_m, area, delays, ap, xs, ys, zs, freq, c, rho, p0, outputs, foci=None, slab=None, fp16=False, directivity=False, aligned=True,
            size=(0.0, 0.0), absorb=0.0, stored=False, pin=None, fp8_pin=None, medium=None, dev=False):
    """pos_m [n, 3] m, delays / ap [F, n], xs / ys / zs grid coordinates [m], outputs = names of FLAG, foci [F, 3] m where the library knows them
    (olx_bf_solve), slab = (x_begin, x_count), aligned: flat axis-aligned elements of equal `size` [m], pin / fp8_pin = OLX_FIELD_VARIANT /
    OLX_FP8_CORRECTION, medium = (marched, one-sum, non-trivial planes, layers, planes per layer) of a heterogeneous plan."""
    n, F = len(pos_m), len(delays)
    xb, xc = slab or (0, len(xs))
    flags = sum(FLAG[o] for o in outputs) | (FLAG["fp16"] if fp16 else 0) | (FLAG["directivity"] if directivity else 0)
    keep = [_d(np.asarray(pos_m).T), _d(area), _d(delays), _d(ap), _d([xs[0], ys[0], zs[0]]), _d([xs[1] - xs[0], ys[1] - ys[0], zs[1] - zs[0]]),
            _i([len(xs), len(ys), len(zs)]), _i([int(aligned), int(stored)]), _d([size[0], size[1], absorb])]
    fo = _d(foci) if foci is not None else (None, None)
    med = _i(medium) if medium is not None else (None, None)
    buf = ctypes.create_string_buffer(1024)
    (_, posp), (_, arp), (_, dp), (_, app), (_, op), (_, hp), (_, gnp), (_, mp), (_, ep) = keep
    length = planq(dev).olq_variant(n, posp, arp, F, dp, app, fo[1], op, hp, gnp, xb, xc, ctypes.c_double(freq), ctypes.c_double(c), ctypes.c_double(rho),
                                    ctypes.c_double(p0), ctypes.c_uint(flags), mp, ep, pin.encode() if pin else None, fp8_pin.encode() if fp8_pin else None,
                                    med[1], buf, len(buf))
    assert 0 < length < len(buf), length
    return buf.value.decode()
