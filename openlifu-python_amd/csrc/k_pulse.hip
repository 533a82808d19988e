// kernel 2p (field_pulse_k): pulsed (tone-burst) field -- peak positive / peak negative pressure over a sampled time axis.
// gfx950 (CDNA4, wave64) only.  Definition: DESIGN.md section 2 ("pulsed model"), fp64 oracle tests/pulsed_oracle.py.
//
// For focus f, voxel v and element e, with d_e = max(|r_v - r_e|, min(spacing) / 2), w_e = a_e P0 S_e / lambda and absorption a [Np/m]:
//     drive     s_e(t) = a_e P0 sin(2 pi f0 (t - tau~_e)) for 0 <= t - tau~_e < T,  T = cycles / f0,  tau~_e = floor(tau_e / dt) dt
//     field     p(v, t) = sum_e w_e exp(-a d_e) / d_e cos(2 pi f0 (t - t_e)) 1[0 <= t - t_e < T],   t_e = tau~_e + d_e / c
//     samples   t_k = k dt, k = 0 .. n_t - 1
//     outputs   p_max = max(0, max_k p(v, t_k)),  p_min = max(0, -min_k p(v, t_k)),  intensity = 1e-4 p_min^2 / (2 rho c)
// Element e is active at samples k0_e <= k < k1_e, k0_e = m_e + ceil(q_e), k1_e = m_e + ceil(q_e + T / dt), m_e = floor(tau_e / dt),
// q_e = d_e / (c dt).  Those two integers are formed in fp64 (distance, q, ceil): a 1-ulp fp32 error in t_e / dt moves a whole element
// term in or out of a sample, ~1/N of the focal peak.  Everything else is fp32.
//
// Between consecutive arrivals / burst ends the complex envelope is constant:
//     p(v, t_k) = Re(e^{j theta_k} C_k),  C_k = sum_{e active at k} c_e,  c_e = w_e exp(-a d_e) / d_e e^{-j phi_e}
// with the phases relative to a per-voxel time origin K (the first sample of the voxel's window): theta_k = 2 pi f0 dt (k - K),
// phi_e = 2 pi frac(f0 dt (m_e - K + q_e)) -- fp64 up to the fractional part, so the fp32 phase error does not grow with t_e.
// One wave per voxel: every lane walks elements lane, lane + 64, ...:
//   1. window [K, K_end): min / max of the arrival and burst-end samples from fp32 distances (2 samples of slack), clipped to [0, n_t);
//   2. per LDS pass of PULSE_L samples: scatter +c_e at sample k0_e and -c_e at k1_e into a difference array (ds_add_f32; samples
//      before the pass go to its slot 0, samples after it are dropped), prefix-scan it across the wave (21 contiguous samples per lane,
//      then a wave scan of the lane totals), evaluate p at every sample of the pass and keep the lane's max / min;
//   3. wave max / min, one lane stores.
// Two opt-in instantiations of the same source ("pulse intensity integral" and "traces"; fp64 oracle
// tests/pulsed_wave_oracle.py); <false, false> is the kernel above (every addition sits under `if constexpr`):
//   PII    the lane also sums p^2 over its valid samples of all passes (fp32), one wave sum at the end, lane 0 stores
//          pii_out = 1e-4 dt / (rho c) sum_k p(v, t_k)^2 [J/cm^2];
//   TRACE  one wave per (point, focus) instead of per voxel, v from a voxel-index list: the lanes store p at their valid samples between
//          the first arrival and the last burst end (both fp64) to trace[(f n_points + i) n_t + k] and no volume; the launcher zeroes the
//          trace first, so every other sample is an exact 0.
//   RESP   drive impulse responses (olx_field_pulse_response; DESIGN.md section 2 "drive taps", section 5.16; fp64 oracle
//          tests/pulsed_response_oracle.py): the elements are split into classes of identical taps; per pass and per class in turn, on the
//          same two LDS arrays, the class's elements are scattered and scanned as above, the envelope C is written back to LDS and every
//          lane applies the class's taps gamma[m] = g[m] e^{-j 2 pi frac(f0 dt m)} to its 21 samples, C'_k += gamma[m] C_{k-m} in ascending
//          m with fused multiply-adds (a window of 21 registers slides back one sample per tap, one LDS read each); C' adds up over the
//          classes from 0 and p = Re(e^{j theta_k} C'_k) is evaluated once.  Consecutive passes overlap by H = M_max - 1 samples (the
//          history of the first outputs of a pass); the window's upper end and the trace's last burst end grow by H.
// Single-pass capacity: PULSE_L = 64 x 21 = 1344 samples per voxel window (20 cycles at 400 kHz on a 0.25 mm grid with the default
// dt = 0.5 x 0.25 mm / 1500 m/s: T / dt = 600 samples + the arrival spread of a 256-element array, ~1100 in all).  Longer windows take
// ceil(window / 1344) passes, each re-walking the elements (the time axis is split, nothing else changes).
#include "k_types.hip.h"
#include "olx_ctx.h"
#include "olx_launch.h"

namespace olx {

constexpr int PULSE_SEG = 21;                    // contiguous samples per lane and pass (odd: the 64 lanes' segments start on distinct LDS banks)
constexpr int PULSE_L = 64 * PULSE_SEG;          // samples per LDS pass
constexpr int PULSE_WAVES = 4;                   // waves per block, one voxel each (2 x 1344 floats = 10.5 KiB of LDS per wave)

// wave-level ordering of LDS traffic between the scatter, scan and clear phases (the lanes of one wave read each other's samples)
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
}

// per (focus, element): { x, y, z [m], m_e = floor(tau_e / dt) } fp64 and w_e = a_e P0 S_e / lambda fp32
__global__ __launch_bounds__(256) void pulse_table_k(const double* __restrict__ pos, const double* __restrict__ area, const double* __restrict__ delays,
                                                     const double* __restrict__ apod, int n, int n_foci, double dt, double wscale,
                                                     double4* __restrict__ tab, float* __restrict__ w) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * n_foci) return;
    const int e = t % n;
    tab[t] = make_double4(pos[e], pos[n + e], pos[2 * n + e], floor(delays[t] / dt));
    w[t] = (float)(apod[t] * area[e] * wscale);
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// RESP: p and the rotation's real part with their roundings written out (products rounded, then the difference / one fused multiply-add):
// the forms the plain instantiations compile to.  Left to the compiler, the RESP instantiations contract them differently from one
// another, and a trace would not carry the bits of the volumes.
__device__ __forceinline__ float pulse_resp_p(float er, float ei, float xr, float xi) {
#pragma clang fp contract(off)
    return er * xr - ei * xi;
}
__device__ __forceinline__ float pulse_resp_rot(float er, float ei, float c, float s) {
#pragma clang fp contract(off)
    const float t = ei * s;
    return fmaf(er, c, -t);
}

// RESP: what olx_field_pulse_response adds to the arguments; empty without it (the plain instantiations take nothing more)
template <bool RESP> struct PulseRespArgs {
    const int* tab;       // [n_el] class of each element, then [n_classes + 1] first tap of each class in gam
    const float* gam;     // [n_taps][2] gamma (re, im)
    int n_classes, n_taps, hist;      // hist = M_max - 1
};
template <> struct PulseRespArgs<false> {};

// TRACE: pmin_out is the trace buffer [n_foci][n_points][n_t], points the voxel indices, pmax_out / inten_out / pii_out unused
template <bool PII, bool TRACE, bool RESP>
__global__ __launch_bounds__(64 * PULSE_WAVES) void field_pulse_k(const double4* __restrict__ tab, const float* __restrict__ wtab, const PulseParams P,
                                                                  float* __restrict__ pmin_out, float* __restrict__ pmax_out, float* __restrict__ inten_out,
                                                                  float* __restrict__ pii_out, const long long* __restrict__ points, int n_points,
                                                                  const PulseRespArgs<RESP> R) {
    __shared__ float lds[PULSE_WAVES][2][PULSE_L];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long w = (long long)blockIdx.x * PULSE_WAVES + wave;      // the wave's voxel, or its entry of the point list
    if (w >= (TRACE ? (long long)n_points : P.vox)) return;            // (whole waves: nothing below synchronises across waves)
    long long v = w;
    if constexpr (TRACE) {
        v = points[w];
        if (!OLX_IN(v, P.vox, 5)) return;
    }
    const int f = blockIdx.y;
    float* re = lds[wave][0];
    float* im = lds[wave][1];
    const int plane = P.ny * P.nz;
    const int i = (int)(v / plane), j = (int)((v % plane) / P.nz), k = (int)(v % P.nz);
    const double px = P.ox + i * P.hx, py = P.oy + j * P.hy, pz = P.oz + k * P.hz;
    const double4* T = tab + (size_t)f * P.n_el;
    const float* W = wtab + (size_t)f * P.n_el;

    // 1. the voxel's window of samples (fp32 distances: only its ends move, by the slack)
    float umin = 3.0e38f, umax = -3.0e38f;
    for (int e = lane; e < P.n_el; e += 64) {
        if (W[e] == 0.f) continue;
        const double4 el = T[e];
        const float dx = (float)(px - el.x), dy = (float)(py - el.y), dz = (float)(pz - el.z);
        const float d = fmaxf(sqrtf(fmaf(dx, dx, fmaf(dy, dy, dz * dz))), P.dmin_f);
        const float u = (float)el.w + d * P.inv_cdt_f;
        umin = fminf(umin, u); umax = fmaxf(umax, u);
    }
    umin = wave_min(umin); umax = wave_max(umax);
    const long long vf = (long long)f * P.vox + v;
    if (umin > umax) {                            // no driven element
        if constexpr (!TRACE) {
            if (lane == 0 && OLX_IN(vf, P.vox * P.n_foci, 6)) {
                pmin_out[vf] = 0.f; if (pmax_out) pmax_out[vf] = 0.f; if (inten_out) inten_out[vf] = 0.f;
                if constexpr (PII) pii_out[vf] = 0.f;
            }
        }
        return;
    }
    const double lo = fmax(floor((double)umin) - 2.0, 0.0);
    double hi = fmin(ceil((double)umax + P.tdt) + 2.0, (double)P.n_t);          // exclusive
    int H = 0, n_cls = 1;                         // RESP: samples of history a pass carries in front of its outputs, classes
    if constexpr (RESP) {
        H = R.hist; n_cls = R.n_classes;
        hi = fmin(ceil((double)umax + P.tdt) + 2.0 + H, (double)P.n_t);
    }

    float pmax = 0.f, pmin = 0.f;                 // (samples outside the window are 0: they bound both from the zero side)
    float e2 = 0.f;                               // PII: the lane's sum of p^2 over its samples of all passes
    float* const trace = pmin_out + ((long long)f * n_points + w) * P.n_t;       // TRACE: this (focus, point)'s row
    const int s0 = lane * PULSE_SEG;
#pragma unroll
    for (int s = 0; s < PULSE_SEG; ++s) { re[s0 + s] = 0.f; im[s0 + s] = 0.f; }
    // RESP: a pass starts H samples before its first output (before `lo` every C is 0) and advances by PULSE_L - H
    for (double base = RESP ? lo - H : lo; RESP ? base + H < hi : base < hi; base += RESP ? PULSE_L - H : PULSE_L) {
        double kbeg = 1.0e300, kend = -1.0e300;   // TRACE: first arrival, last burst end (the fp64 integers; the same in every pass)
        float sr[PULSE_SEG], si[PULSE_SEG];
        float cr, ci;
        float ar[RESP ? PULSE_SEG : 1], ai[RESP ? PULSE_SEG : 1];      // RESP: C' of the lane's samples, summed over the classes
        if constexpr (RESP) {
#pragma unroll
            for (int s = 0; s < PULSE_SEG; ++s) { ar[s] = 0.f; ai[s] = 0.f; }
        }
        int r = 0;                                // RESP: the class whose turn it is (without RESP: one turn, no loop)
        do {                                      // (2a, 2b and 2b' are its body, kept at the pass's indentation: without RESP they are the pass)
        wave_lds_sync();
        // 2a. scatter the element terms into the difference array of this pass
        for (int e = lane; e < P.n_el; e += 64) {
            const float we = W[e];
            if (we == 0.f) continue;
            if constexpr (RESP) {
                if (!OLX_IN(e, P.n_el, 7) || R.tab[e] != r) continue;      // another class's turn
            }
            const double4 el = T[e];
            const double dx = px - el.x, dy = py - el.y, dz = pz - el.z;
            const double d = fmax(sqrt(fma(dx, dx, fma(dy, dy, dz * dz))), P.dmin);
            const double q = d * P.inv_cdt;
            const double k0 = el.w + ceil(q), k1 = el.w + ceil(q + P.tdt);
            if constexpr (TRACE) { kbeg = fmin(kbeg, k0); kend = fmax(kend, k1); }
            if (k0 >= base + PULSE_L || k1 <= base || k1 <= k0) continue;      // after this pass, or over before it: nothing here
            double cyc = P.f0dt * ((el.w - lo) + q);
            cyc -= floor(cyc);
            const float ph = (float)cyc;
            const float df = (float)d;
            float a = we * __builtin_amdgcn_rcpf(df);
            if (P.absorb > 0.f) a *= __expf(-P.absorb * df);
            const float cr = a * __builtin_amdgcn_cosf(ph), ci = -a * __builtin_amdgcn_sinf(ph);
            const int i0 = k0 <= base ? 0 : (int)(k0 - base);
            if (OLX_IN(i0, PULSE_L, 0)) { atomicAdd(&re[i0], cr); atomicAdd(&im[i0], ci); }
            if (k1 < base + PULSE_L) {
                const int i1 = (int)(k1 - base);
                if (OLX_IN(i1, PULSE_L, 1)) { atomicAdd(&re[i1], -cr); atomicAdd(&im[i1], -ci); }
            }
        }
        wave_lds_sync();
        // 2b. prefix scan: the lane's own segment, then the exclusive scan of the segment totals across the wave
        float tr = 0.f, ti = 0.f;
#pragma unroll
        for (int s = 0; s < PULSE_SEG; ++s) {
            sr[s] = re[s0 + s]; si[s] = im[s0 + s];
            tr += sr[s]; ti += si[s];
            sr[s] = tr; si[s] = ti;
        }
        cr = tr; ci = ti;                        // inclusive scan of the totals
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float ur = __shfl_up(cr, o), ui = __shfl_up(ci, o);
            if (lane >= o) { cr += ur; ci += ui; }
        }
        cr -= tr; ci -= ti;                      // ... exclusive: the carry into this lane's segment
        wave_lds_sync();
        if constexpr (RESP) {
            // 2b'. C back to LDS (the lanes read each other's), then the class's taps over the lane's samples: wr / wi hold C_{k-m}
            float wr[PULSE_SEG], wi[PULSE_SEG];
#pragma unroll
            for (int s = 0; s < PULSE_SEG; ++s) {
                wr[s] = cr + sr[s]; wi[s] = ci + si[s];
                if (OLX_IN(s0 + s, PULSE_L, 9)) { re[s0 + s] = wr[s]; im[s0 + s] = wi[s]; }
            }
            wave_lds_sync();
            int g0 = 0, g1 = 0;
            if (OLX_IN(P.n_el + r + 1, P.n_el + R.n_classes + 1, 7)) { g0 = R.tab[P.n_el + r]; g1 = R.tab[P.n_el + r + 1]; }
            for (int g = g0; g < g1; ++g) {       // tap m = g - g0, ascending
                if (!OLX_IN(g, R.n_taps, 8)) break;
                const float gr = R.gam[2 * g], gi = R.gam[2 * g + 1];
#pragma unroll
                for (int s = 0; s < PULSE_SEG; ++s) {
                    ar[s] = fmaf(gr, wr[s], ar[s]); ar[s] = fmaf(-gi, wi[s], ar[s]);
                    ai[s] = fmaf(gr, wi[s], ai[s]); ai[s] = fmaf(gi, wr[s], ai[s]);
                }
#pragma unroll
                for (int s = PULSE_SEG - 1; s > 0; --s) { wr[s] = wr[s - 1]; wi[s] = wi[s - 1]; }
                const int h = s0 - 1 - (g - g0);      // the sample before the window (before the pass: history nobody reads, or 0)
                const bool in = h >= 0 && OLX_IN(h, PULSE_L, 10);
                wr[0] = in ? re[h] : 0.f; wi[0] = in ? im[h] : 0.f;
            }
            wave_lds_sync();
        }
#pragma unroll
        for (int s = 0; s < PULSE_SEG; ++s) { re[s0 + s] = 0.f; im[s0 + s] = 0.f; }     // (cleared for the next pass)
        } while (RESP && ++r < n_cls);
        // 2c. p at the pass's samples: theta_k = 2 pi f0 dt (k - lo), exact at the segment's first sample, rotated by 2 pi f0 dt after it
        const double kfirst = base + s0;
        double cyc = P.f0dt * (kfirst - lo);
        cyc -= floor(cyc);
        float er = __builtin_amdgcn_cosf((float)cyc), ei = __builtin_amdgcn_sinf((float)cyc);
        const int nvalid = (int)fmin(fmax(hi - kfirst, 0.0), (double)PULSE_SEG);
        int sbeg = 0, send = nvalid;              // TRACE: the valid samples at which an element is or has been active
        if constexpr (TRACE) {
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) { kbeg = fmin(kbeg, __shfl_xor(kbeg, o)); kend = fmax(kend, __shfl_xor(kend, o)); }
            if constexpr (RESP) kend += H;        // (the last tap of the last burst)
            sbeg = (int)fmin(fmax(kbeg - kfirst, 0.0), (double)PULSE_SEG);
            send = min(nvalid, (int)fmin(fmax(kend - kfirst, 0.0), (double)PULSE_SEG));
        }
        int vbeg = 0;                             // RESP: the lane's first sample past the pass's history
        if constexpr (RESP) { vbeg = min(max(H - s0, 0), PULSE_SEG); sbeg = max(sbeg, vbeg); }
#pragma unroll
        for (int s = 0; s < PULSE_SEG; ++s) {
            float p;
            if constexpr (RESP) p = pulse_resp_p(er, ei, ar[s], ai[s]);
            else p = er * (cr + sr[s]) - ei * (ci + si[s]);
            if constexpr (TRACE) {
                if (s >= sbeg && s < send) {
                    const long long kk = (long long)kfirst + s;
                    if (OLX_IN(kk, P.n_t, 4)) trace[kk] = p;
                }
            } else if (RESP ? s >= vbeg && s < nvalid : s < nvalid) {
                pmax = fmaxf(pmax, p); pmin = fminf(pmin, p);
                if constexpr (PII) e2 = fmaf(p, p, e2);
            }
            float nr;
            if constexpr (RESP) nr = pulse_resp_rot(er, ei, P.rot_c, P.rot_s);
            else nr = er * P.rot_c - ei * P.rot_s;
            ei = fmaf(er, P.rot_s, ei * P.rot_c);
            er = nr;
        }
    }
    if constexpr (TRACE) return;
    pmax = wave_max(pmax); pmin = wave_min(pmin);
    if constexpr (PII) e2 = wave_sum(e2);
    if (lane == 0 && OLX_IN(vf, P.vox * P.n_foci, 2)) {
        const float pn = 0.f - pmin;          // (+0 where nothing arrived)
        pmin_out[vf] = pn;
        if (pmax_out) pmax_out[vf] = pmax;
        if (inten_out) inten_out[vf] = P.inten_scale * pn * pn;
    }
    if constexpr (PII) {
        if (lane == 0 && OLX_IN(vf, P.vox * P.n_foci, 3)) pii_out[vf] = P.pii_scale * e2;
    }
}

OLX_BOUNDS_READER(pulse)

}  // namespace olx

using namespace olx;

static void launch_pulse_table(olx_ctx* c) {
    const int fn = c->n_el * c->plan_foci;
    hipLaunchKernelGGL(pulse_table_k, dim3((fn + 255) / 256), dim3(256), 0, c->stream, c->d_pos, c->d_area, c->d_delays, c->d_apod, c->n_el,
                       c->plan_foci, c->pulse_plan_dt, c->p0_pa * c->freq / c->c, c->d_ptab, c->d_pw);      // (the dt of the plan, not of a later olx_field_pulse)
}

// the plan's response (olx_field_pulse_response) as the RESP instantiations take it
static PulseRespArgs<true> resp_args(const olx_ctx* c) {
    PulseRespArgs<true> R;
    R.tab = c->d_presp_tab; R.gam = c->d_presp_gam;
    R.n_classes = c->presp_classes; R.n_taps = c->presp_taps; R.hist = c->presp_hist;
    return R;
}

void olx_launch_pulse(olx_ctx* c, float* pm) {
    const PulseParams& P = c->pulse;
    launch_pulse_table(c);
    const dim3 grid((unsigned)((P.vox + PULSE_WAVES - 1) / PULSE_WAVES), c->plan_foci);
    float* const px = (c->flags & OLX_OUT_PMAX) ? (float*)c->d_pmax : nullptr;
    float* const it = (c->flags & OLX_OUT_INTENSITY) ? (float*)c->d_inten : nullptr;
    if (c->presp_classes > 0) {
        if (c->flags & OLX_OUT_PII)
            hipLaunchKernelGGL((field_pulse_k<true, false, true>), grid, dim3(64 * PULSE_WAVES), 0, c->stream, c->d_ptab, c->d_pw, P, pm, px, it,
                               (float*)c->d_pii, (const long long*)nullptr, 0, resp_args(c));
        else
            hipLaunchKernelGGL((field_pulse_k<false, false, true>), grid, dim3(64 * PULSE_WAVES), 0, c->stream, c->d_ptab, c->d_pw, P, pm, px, it,
                               (float*)nullptr, (const long long*)nullptr, 0, resp_args(c));
    } else if (c->flags & OLX_OUT_PII)
        hipLaunchKernelGGL((field_pulse_k<true, false, false>), grid, dim3(64 * PULSE_WAVES), 0, c->stream, c->d_ptab, c->d_pw, P, pm, px, it, (float*)c->d_pii,
                           (const long long*)nullptr, 0, PulseRespArgs<false>{});
    else
        hipLaunchKernelGGL((field_pulse_k<false, false, false>), grid, dim3(64 * PULSE_WAVES), 0, c->stream, c->d_ptab, c->d_pw, P, pm, px, it, (float*)nullptr,
                           (const long long*)nullptr, 0, PulseRespArgs<false>{});
}

void olx_launch_pulse_trace(olx_ctx* c, int n_points) {
    launch_pulse_table(c);      // (the caller has zeroed c->d_ptrace on the stream)
    const dim3 grid((unsigned)((n_points + PULSE_WAVES - 1) / PULSE_WAVES), c->plan_foci);
    if (c->presp_classes > 0)
        hipLaunchKernelGGL((field_pulse_k<false, true, true>), grid, dim3(64 * PULSE_WAVES), 0, c->stream, c->d_ptab, c->d_pw, c->pulse, (float*)c->d_ptrace,
                           (float*)nullptr, (float*)nullptr, (float*)nullptr, (const long long*)c->d_ptrace_vox, n_points, resp_args(c));
    else
        hipLaunchKernelGGL((field_pulse_k<false, true, false>), grid, dim3(64 * PULSE_WAVES), 0, c->stream, c->d_ptab, c->d_pw, c->pulse, (float*)c->d_ptrace,
                           (float*)nullptr, (float*)nullptr, (float*)nullptr, (const long long*)c->d_ptrace_vox, n_points, PulseRespArgs<false>{});
}
