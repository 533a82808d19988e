"""Case table of the full-wave drive tests (tests/test_gpu_fullwave_drive.py, tests/test_fullwave_drive_host.py): each case is the input of
ONE run on the grid the device sees, in element-factored form -- entries (voxel, element, amplitude per unit A), per-element (A, tau), a
class per element and the classes' drive taps -- handed unchanged to the C-ABI and, with the taps expanded into shifted entries
(tests/fullwave_drive_oracle.py ``expand``), to the fp64 oracles.  The media and the element builders are those of tests/fullwave_cases.py
and tests/fullwave_aperture_cases.py.  Delays are in units of dt, off the half-integers: every case keeps activity_margin >= 1e-3 (a tap
shifts by whole steps, which leaves the margin alone).  Oracle results are computed once per case and shared."""
import functools

import numpy as np

import fullwave_aperture_cases as ac
import fullwave_aperture_oracle as ao
import fullwave_cases as fc
import fullwave_drive_oracle as do
import fullwave_lockin_oracle as lo
import fullwave_oracle as fo
import fullwave_pml_oracle as po

FREQ = fc.FREQ


def tone_taps(M, dt, phase=0.3, scale=1.0):
    """M Hann-windowed taps of a tone at FREQ: a band-pass response around the drive frequency"""
    m = np.arange(M, dtype=np.float64)
    w = 0.5 * (1.0 - np.cos(2.0 * np.pi * (m + 1.0) / (M + 1.0)))
    return scale * w * np.cos(2.0 * np.pi * FREQ * dt * m + phase)


def _points(base, pos, A, tau_steps, cls, taps, layer="sponge"):
    """an element-factored case of trilinear point elements out of a fullwave_cases._case ``base``"""
    hh = np.asarray(base["h"])
    ijk, el, amp = [], [], []
    for e, p in enumerate(pos):
        q, a, _ = fo.monopole_entries(np.asarray([p], dtype=np.float64) * hh, (0, 0, 0), hh, [1.0], [0.0], base["c"], base["freq"], base["dt"], base["n"])
        ijk.append(q); el.append(np.full(len(a), e, dtype=np.int32)); amp.append(a)
    k = {key: base[key] for key in ("n", "h", "c", "rho", "alpha", "c_ref", "pml", "pml_alpha", "dt", "steps", "freq", "cycles", "ramp", "trace")}
    k.update(eijk=np.concatenate(ijk), el=np.concatenate(el), amp1=np.concatenate(amp), A=np.asarray(A, dtype=np.float64),
             tau_e=np.asarray(tau_steps, dtype=np.float64) * base["dt"], cls=np.asarray(cls, dtype=np.int32), taps=[np.asarray(t, dtype=np.float64) for t in taps],
             layer=layer, apertures=None)
    return k


def _apertures(base, cls, taps, name=None):
    """an element-factored case out of a fullwave_aperture_cases._case ``base``: the oracle's weights are its entries; ``name`` (a case of
    fullwave_aperture_cases) lets the device form the weights itself (olx_fullwave_apertures)"""
    row, ijk, wt = ao.aperture_table(base["centre"], base["u"], base["v"], base["size"], base["nw"], base["nl"], ac.ORIGIN, base["h"], base["n"])
    E = len(base["A"])
    eijk, amp, _ = ao.expand(row, ijk, wt, np.ones(E), np.zeros(E), base["c"], base["freq"], base["dt"], base["h"], base["n"])
    k = {key: base[key] for key in ("n", "h", "c", "rho", "alpha", "c_ref", "pml", "pml_alpha", "dt", "steps", "freq", "cycles", "ramp", "trace")}
    k.update(eijk=eijk, el=np.repeat(np.arange(E, dtype=np.int32), np.diff(row)), amp1=amp, A=base["A"], tau_e=base["tau"], cls=np.asarray(cls, dtype=np.int32),
             taps=[np.asarray(t, dtype=np.float64) for t in taps], layer="sponge", apertures=name)
    return k


def _cases():
    out = {}
    # (a) uniform water 24^3, 6-voxel layers, 3 off-voxel point elements on interior voxels, one class of 7 taps; (g) the same under split layers
    pos_a, A_a, tau_a = [(9.3, 11.6, 8.25), (13.7, 10.4, 8.5), (11.5, 14.2, 9.75)], [1.0, 0.7, 0.85], [0.2, 7.3, 3.4]
    base = fc._case((24, 24, 24), 0.5e-3, fc.WATER, 6, pos_a, A_a, tau_a, 220, trace=[(12, 12, 15), (8, 14, 16), (0, 0, 0)])
    g7 = tone_taps(7, base["dt"])
    out["a_one_class"] = _points(base, pos_a, A_a, tau_a, [0, 0, 0], [g7])
    out["g_split_layers"] = _points(base, pos_a, A_a, tau_a, [0, 0, 0], [g7], layer="pml")
    # (f) taps [1.0]: the bare drive
    out["f_identity"] = _points(base, pos_a, A_a, tau_a, [0, 0, 0], [[1.0]])
    # (b) the layered medium on the odd anisotropic grid, a ramp; classes of 1, 2 and 33 taps and [1.0] for the element without a response; element 0
    # starts before step 0 with the 33 taps reaching back there, element 4's burst still runs at the end of the run, element 3 has A = 0
    n, h = (37, 29, 43), (0.4e-3, 0.5e-3, 0.3e-3)
    pos = [(12.4, 9.7, 8.2), (12.6, 9.2, 8.9), (24.0, 18.0, 8.0), (20.5, 12.5, 9.5), (8.3, 20.1, 7.7)]
    A, tau = [1.0, 0.8, 0.6, 0.0, 0.9], [-5.3, 11.7, 25.2, 3.3, 330.8]
    base = fc._case(n, h, fc.layered(n), 6, pos, A, tau, 400, cycles=4.0, ramp=1.5, trace=[(18, 14, 30), (13, 10, 16), (36, 28, 42)])
    out["b_layered"] = _points(base, pos, A, tau, [2, 1, 0, 3, 2], [[0.7], [0.6, -0.35], tone_taps(33, base["dt"], 1.1, 0.4), [1.0]])
    # (c) aperture elements with two classes (the device forms the weights)
    base = ac.CASES["axis_aligned"]
    out["c_apertures"] = _apertures(base, [0, 1, 1, 0], [tone_taps(5, base["dt"], 0.0, 0.9), [0.25, 0.5, 0.25]], name="axis_aligned")
    # (d) one element with 256 taps on 16^3
    pos_d = [(7.0, 8.0, 6.4)]
    base = fc._case((16, 16, 16), 0.5e-3, fc.WATER, 3, pos_d, [1.0], [0.3], 330, cycles=3.0, trace=[(8, 8, 10)])
    out["d_256_taps"] = _points(base, pos_d, [1.0], [0.3], [0], [tone_taps(256, base["dt"], 0.7, 0.05)])
    # (e) 300 one-point elements on 32^3, each its own class of 1 .. 3 taps: n_classes = n_el, more than one block of lanes
    base = ac._many(300)
    rng = np.random.default_rng(20)
    out["e_own_classes"] = _apertures(base, np.arange(300), [rng.uniform(-1.0, 1.0, 1 + e % 3) for e in range(300)])
    return out


CASES = _cases()
NAMES = sorted(CASES)
for _name, _k in CASES.items():
    assert fo.activity_margin(_k["tau_e"], _k["cycles"] / _k["freq"], _k["dt"]) >= 1e-3, _name


def table(name):
    """the fp64 drive table s[steps, n_el] of the case, from the definition"""
    k = CASES[name]
    return do.drive_table(k["A"], k["tau_e"], k["cls"], k["taps"], k["freq"], k["cycles"], k["ramp"], k["dt"], k["steps"])


def tap_norm(name):
    """sum |g| of each element's class"""
    k = CASES[name]
    return np.array([np.abs(k["taps"][c]).sum() for c in k["cls"]])


def entries(name, taps=True):
    """the oracle's per-entry table (ijk, amp, tau): the taps expanded into shifted entries, or (``taps=False``) the bare sources"""
    k = CASES[name]
    base = (k["eijk"], k["amp1"] * k["A"][k["el"]], k["tau_e"][k["el"]], k["el"])
    return do.expand(base, k["cls"], k["taps"], k["dt"]) if taps else base[:3]


def _simulate(name, taps, trace=None):
    k = CASES[name]
    ijk, amp, tau = entries(name, taps)
    sim = po.simulate if k["layer"] == "pml" else fo.simulate
    return sim(k["n"], k["h"], k["c"], k["rho"], k["alpha"], k["c_ref"], k["pml"], k["pml_alpha"], k["dt"], k["steps"], ijk, amp, tau, k["freq"], k["cycles"],
               k["ramp"], trace_ijk=k["trace"] if trace is None else trace)


@functools.lru_cache(maxsize=None)
def reference(name, taps=True):
    ref = _simulate(name, taps)
    for v in ref.values():
        v.setflags(write=False)
    return ref


def device_entries(ctx, name):
    """(linear voxels, elements, amplitude per unit A) as the device takes them; plans the case"""
    k = CASES[name]
    ctx.fullwave_plan(k["h"], k["n"], k["c"], k["rho"], k["alpha"], k["c_ref"], k["pml"], k["pml_alpha"], k["dt"], layer_model=k["layer"])
    if k["apertures"] is not None:
        return ac.device_table(ctx, k["apertures"])
    return fc.lin(k["eijk"], k["n"]), k["el"], k["amp1"]


def set_sources(ctx, name, response=True, A=None, tau=None):
    """plan, olx_fullwave_sources_elements and (``response``) olx_fullwave_drive_response of the case"""
    k = CASES[name]
    vox, el, amp = device_entries(ctx, name)
    ctx.fullwave_sources_elements(vox, el, amp, k["A"] if A is None else A, k["tau_e"] if tau is None else tau, k["freq"], k["cycles"], k["ramp"], k["steps"],
                                  points=fc.lin(k["trace"], k["n"]))
    if response:
        ctx.fullwave_drive_response(k["cls"], k["taps"])


def run(ctx, name, split=None, psq=True):
    k = CASES[name]
    if split is None:
        ctx.fullwave_run(0, k["steps"], psq=psq)
    else:
        ctx.fullwave_run(0, split, psq=psq)
        ctx.fullwave_run(split, k["steps"] - split, psq=psq)
    return ctx.fullwave_fetch()


def run_device(ctx, name, response=True, split=None):
    """The case through the C-ABI -> (p_max, p_min, psq, trace [steps, P])."""
    set_sources(ctx, name, response)
    return run(ctx, name, split)


# ---- steady state: case (a)'s elements driven through the end of the run, one class on all elements, the lock-in over the last third ----
def _steady():
    pos, A, tau = [(9.3, 11.6, 8.25), (13.7, 10.4, 8.5), (11.5, 14.2, 9.75)], [1.0, 0.7, 0.85], [0.2, 7.3, 3.4]
    steps = 360
    base = fc._case((24, 24, 24), 0.5e-3, fc.WATER, 6, pos, A, tau, steps, cycles=1.0, ramp=2.0)
    base["cycles"] = float(np.ceil(FREQ * steps * base["dt"]) + 1.0)          # the drive lasts through the end of the run
    return _points(base, pos, A, tau, [0, 0, 0], [tone_taps(7, base["dt"], 0.3, 0.5)])


STEADY = _steady()


def steady_window():
    return STEADY["steps"] - STEADY["steps"] // 3, STEADY["steps"] // 3


@functools.lru_cache(maxsize=None)
def steady_reference(taps=True):
    """(C [n], S [n]) of the lock-in oracle over the run of the expanded (or the bare) entries"""
    k = STEADY
    every = np.stack(np.meshgrid(*[np.arange(v) for v in k["n"]], indexing="ij"), axis=-1).reshape(-1, 3)
    base = (k["eijk"], k["amp1"] * k["A"][k["el"]], k["tau_e"][k["el"]], k["el"])
    ijk, amp, tau = do.expand(base, k["cls"], k["taps"], k["dt"]) if taps else base[:3]
    tr = fo.simulate(k["n"], k["h"], k["c"], k["rho"], k["alpha"], k["c_ref"], k["pml"], k["pml_alpha"], k["dt"], k["steps"], ijk, amp, tau, k["freq"], k["cycles"],
                     k["ramp"], trace_ijk=every)["trace"]
    C, S = lo.volume_sums(tr, k["freq"], k["dt"], *steady_window())
    C, S = C.reshape(k["n"]), S.reshape(k["n"])
    C.setflags(write=False); S.setflags(write=False)
    return C, S


def known_answer_deviation(bare, resp):
    """(amplitude, phase [cycles]) deviation of the run with the response from |G| times the bare run's amplitude and its lag shifted by
    -arg G / 2 pi, over the interior voxels where the bare amplitude is at least a tenth of its largest; the amplitude as a fraction of |G|"""
    k = STEADY
    nw = steady_window()[1]
    G = do.gain(k["taps"][0], k["freq"], k["dt"])
    q = k["pml"]
    crop = (slice(q, -q),) * 3
    a0, p0 = lo.amplitude_phase(np.asarray(bare[0], dtype=np.float64)[crop], np.asarray(bare[1], dtype=np.float64)[crop], nw)
    a1, p1 = lo.amplitude_phase(np.asarray(resp[0], dtype=np.float64)[crop], np.asarray(resp[1], dtype=np.float64)[crop], nw)
    at = a0 >= 0.1 * a0.max()
    d_amp = float(np.abs(a1[at] / a0[at] - abs(G)).max() / abs(G))
    shift = (p1[at] - p0[at]) + np.angle(G) / (2.0 * np.pi)
    d_ph = float(np.abs((shift + 0.5) % 1.0 - 0.5).max())
    return d_amp, d_ph


def run_device_steady(ctx, response=True):
    k = STEADY
    ctx.fullwave_plan(k["h"], k["n"], k["c"], k["rho"], k["alpha"], k["c_ref"], k["pml"], k["pml_alpha"], k["dt"])
    ctx.fullwave_sources_elements(fc.lin(k["eijk"], k["n"]), k["el"], k["amp1"], k["A"], k["tau_e"], k["freq"], k["cycles"], k["ramp"], k["steps"])
    if response:
        ctx.fullwave_drive_response(k["cls"], k["taps"])
    w = steady_window()
    ctx.fullwave_lockin(k["freq"], w[0], w[1], volume=True)
    ctx.fullwave_run(0, k["steps"])
    vc, vs, _, _ = ctx.fullwave_fetch_lockin()
    return vc, vs
