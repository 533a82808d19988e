// kernel 2ph (field_pulse_med_k): the pulsed (tone-burst) field of kernel 2p through a heterogeneous medium along straight rays.
// gfx950 (CDNA4, wave64) only.  Definition: DESIGN.md section 2 ("Pulsed model through a medium"), fp64 oracle tests/pulsed_medium_oracle.py.
//
// Kernel 2p's model (k_pulse.hip) with the medium on every ray: per voxel v = (i, j, kv) and element e, d' = max(|r_v - g_e|, dmin),
//     A_e = 0 if z_v == z_e, else l (a(v) / 2 + sum_{k in K} a_k(crossing_k)),  l = hz d' / |z_v - z_e|        E_e = the same sum over sig = c_ref / c - 1
//     K   = kfirst_e <= k < kv (voxel above the element) | kv < k <= klast_e (below): the host's fp64 plane bounds (kernel 4h's rule)
//     t_e = tau~_e + (d' + E_e) / c_ref,   p(v, t) = sum_e w_e exp(-A_e) / d' cos(2 pi f0 (t - t_e)) 1[0 <= t - t_e < T]
// and p_max, p_min, intensity, PII and the traces as kernel 2p forms them, the intensity and the PII with the voxel's own rho c.
//
// Work map as 2p: one wave per voxel, lanes walk elements lane, lane + 64, ...; difference array in LDS, wave scan, evaluation as 2p.
// What differs:
//   * ONE walk of each ray per (voxel, element).  A ray costs n_planes fp64 bilinear gathers, so q_e = (d' + E_e) / (c_ref dt) (fp64) and the
//     amplitude exp(-A_e) / d' (fp32) are cached in registers per (lane, slot): R = 4 slots for N <= 256, R = 16 for N <= 1024.  The window,
//     k0 / k1, the phase and every LDS pass read the cache (slot r of the arrays is picked by an unrolled chain of selects on the
//     wave-uniform r, never by a run-time index: registers, not scratch).
//   * ALL foci of the launch inside the wave: the ray sums do not depend on the focus, only m_e = floor(tau_e / dt) and w_e do, so the
//     window / scatter / scan part loops over the foci with the cache held (2p: blockIdx.y = focus).
//   * the medium: sig fp64 and a fp32 [Np/m] as compact [plane][i][j] arrays over the non-trivial planes, one load per row of the 2 x 2 stencil (a
//     pre-gathered 2 x 2 stencil of fp64 sig + fp32 a would be 48 bytes per cell, four times the footprint, for gathers that are scattered
//     over the plane either way: the lanes of a wave are different ELEMENTS' crossings of one plane).
// Precision (extends 2p's contract): whether element e is active at sample k is an fp64 decision, which now covers E_e -- sig, the crossing
// coordinates, the bilinear weights, the sum, q_e and the fractional part of the phase are fp64; A_e, exp, amplitudes and the scan fp32.
// The plane loop runs over all held planes with wave-uniform bounds (one voxel per wave: kv is uniform); kfirst_e / klast_e differ per lane
// and are guarded inside it.
//
// Bounds sites of the debug library: 0 / 1 the LDS difference array, 2 / 3 the volume stores (p, PII), 4 the trace, 5 the point list,
// 6 the stores of a voxel without a driven element, 7 sig texels, 8 a texels, 9 the plane list, 10 the plane map, 11 the element records,
// 12 the impedance volume.
#include "k_types.hip.h"
#include "olx_ctx.h"
#include "olx_launch.h"

namespace olx {

constexpr int PM_SEG = 21;                       // contiguous samples per lane and pass (kernel 2p's segmenting)
constexpr int PM_L = 64 * PM_SEG;                // samples per LDS pass
constexpr int PM_WAVES = 4;                      // waves per block, one voxel each

__device__ __forceinline__ void pm_lds_sync() {  // (kernel 2p's wave_lds_sync)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
}

// kernel 2p's table: per (focus, element) { x, y, z [m], m_e = floor(tau_e / dt) } fp64 and w_e = a_e P0 S_e / lambda fp32
__global__ __launch_bounds__(256) void pulse_med_table_k(const double* __restrict__ pos, const double* __restrict__ area, const double* __restrict__ delays,
                                                         const double* __restrict__ apod, int n, int n_foci, double dt, double wscale,
                                                         double4* __restrict__ tab, float* __restrict__ w) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * n_foci) return;
    const int e = t % n;
    tab[t] = make_double4(pos[e], pos[n + e], pos[2 * n + e], floor(delays[t] / dt));
    w[t] = (float)(apod[t] * area[e] * wscale);
}

__device__ __forceinline__ float pm_wave_max(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float pm_wave_min(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float pm_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double pm_wave_maxd(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double pm_wave_mind(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}

// the two neighbours (j, j + 1) of one medium row as ONE load (element-aligned, not vector-aligned); `pair` false: the row has one column
typedef double pm_d2u_t __attribute__((ext_vector_type(2), aligned(8)));
typedef float pm_f2u_t __attribute__((ext_vector_type(2), aligned(4)));
template <class V, class T>
__device__ __forceinline__ void pm_rows(const T* __restrict__ vol, long long o0, long long o1, long long n_ext, bool pair, int site, V& r0, V& r1) {
    if (pair) {
        if (OLX_IN(o0, n_ext, site) && OLX_IN(o0 + 1, n_ext, site)) r0 = *reinterpret_cast<const V*>(vol + o0);
        if (OLX_IN(o1, n_ext, site) && OLX_IN(o1 + 1, n_ext, site)) r1 = *reinterpret_cast<const V*>(vol + o1);
    } else {
        if (OLX_IN(o0, n_ext, site)) r0 = V{vol[o0], vol[o0]};
        if (OLX_IN(o1, n_ext, site)) r1 = V{vol[o1], vol[o1]};
    }
}

// TRACE: pmin_out is the trace buffer [n_foci][n_points][n_t], points the voxel indices, pmax_out / inten_out / pii_out unused
template <int R, bool PII, bool TRACE>
__global__ __launch_bounds__(64 * PM_WAVES) __attribute__((amdgpu_waves_per_eu(R == 4 ? 3 : 2))) void field_pulse_med_k(const double4* __restrict__ tab, const float* __restrict__ wtab, const int2* __restrict__ kb,
                                                                   const double* __restrict__ sig, const float* __restrict__ att,
                                                                   const int* __restrict__ plane_k, const int* __restrict__ plane_of_k,
                                                                   const float* __restrict__ inv2z, const PulseMedParams M,
                                                                   float* __restrict__ pmin_out, float* __restrict__ pmax_out, float* __restrict__ inten_out,
                                                                   float* __restrict__ pii_out, const long long* __restrict__ points, int n_points) {
    __shared__ float lds[PM_WAVES][2][PM_L];
    const PulseParams& P = M.P;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long w = (long long)blockIdx.x * PM_WAVES + wave;        // the wave's voxel, or its entry of the point list
    if (w >= (TRACE ? (long long)n_points : P.vox)) return;            // (whole waves: nothing below synchronises across waves)
    long long v = w;
    if constexpr (TRACE) {
        v = points[w];
        if (!OLX_IN(v, P.vox, 5)) return;
    }
    float* re = lds[wave][0];
    float* im = lds[wave][1];
    const int plane = P.ny * P.nz;
    // (one voxel per wave: its indices are wave-uniform, and so are the plane loop's bounds below)
    const int i = __builtin_amdgcn_readfirstlane((int)(v / plane)), j = __builtin_amdgcn_readfirstlane((int)((v % plane) / P.nz));
    const int kv = __builtin_amdgcn_readfirstlane((int)(v % P.nz));
    const double px = P.ox + i * P.hx, py = P.oy + j * P.hy, pz = P.oz + kv * P.hz;
    const long long nxy = (long long)M.nx * P.ny, n_ext = nxy * M.n_planes;
    const int imax = M.nx - 1, jmax = P.ny - 1, i0max = max(M.nx - 2, 0), j0max = max(P.ny - 2, 0);
    const bool pair = P.ny >= 2;

    // the voxel's own half layer
    double s_own = 0.0;
    float a_own = 0.f;
    {
        const int pq = OLX_IN(kv, P.nz, 10) ? plane_of_k[kv] : -1;
        if (pq >= 0 && OLX_IN(pq, M.n_planes, 9)) {
            const long long o = pq * nxy + (long long)i * P.ny + j;
            if (sig && OLX_IN(o, n_ext, 7)) s_own = 0.5 * sig[o];
            if (att && OLX_IN(o, n_ext, 8)) a_own = 0.5f * att[o];
        }
    }

    // 0. ONE walk of the rays: q_e = (d' + E_e) / (c_ref dt) and exp(-A_e) / d' of the lane's elements into the cache
    double qc[R];
    float ac[R];
#pragma unroll
    for (int s = 0; s < R; ++s) { qc[s] = 0.0; ac[s] = 0.f; }
    const int nr = min(R, (P.n_el + 63) >> 6);
    for (int r = 0; r < nr; ++r) {
        const int e = lane + 64 * r;
        const bool valid = e < P.n_el;
        const int ec = valid ? e : P.n_el - 1;
        double4 el = make_double4(0.0, 0.0, 0.0, 0.0);
        int2 b = make_int2(0, -1);
        if (OLX_IN(ec, P.n_el, 11)) { el = tab[ec]; b = kb[ec]; }
        const double wx = px - el.x, wy = py - el.y, wz = pz - el.z;
        const double d = fmax(sqrt(fma(wx, wx, fma(wy, wy, wz * wz))), P.dmin);
        const bool moving = valid && wz != 0.0;                         // z_v == z_e: A = E = 0
        const double inv_wz = moving ? 1.0 / wz : 0.0;
        // the crossing of plane k in grid index space: (eu, ev) + t (du, dv), t = (z_k - z_e) / (z_v - z_e)
        const double eu = (el.x - P.ox) * M.inv_hx, ev = (el.y - P.oy) * M.inv_hy, du = wx * M.inv_hx, dv = wy * M.inv_hy;
        double ss = s_own;
        float as = a_own;
        for (int p = 0; p < M.n_planes; ++p) {
            const int k = OLX_IN(p, M.n_planes, 9) ? plane_k[p] : kv;
            if (k == kv) continue;                                      // (wave-uniform)
            const bool between = moving && (k < kv ? k >= b.x : k <= b.y);
            if (!between) continue;
            const double t = ((P.oz + k * P.hz) - el.z) * inv_wz;
            const double u = fmin(fmax(fma(t, du, eu), 0.0), (double)imax), vv = fmin(fmax(fma(t, dv, ev), 0.0), (double)jmax);
            const int i0 = min((int)u, i0max), j0 = min((int)vv, j0max);
            const int i1 = min(i0 + 1, imax);
            const double fu = u - i0, fv = vv - j0;
            // (j0 <= ny - 2: the row pair (j0, j0 + 1) is contiguous, one load per row; a single-column grid reads its one value twice)
            const long long o0 = p * nxy + (long long)i0 * P.ny + j0, o1 = p * nxy + (long long)i1 * P.ny + j0;
            // (all four loads issued before the first use; a volume that is absent contributes its zeros)
            pm_d2u_t s0{0.0, 0.0}, s1{0.0, 0.0};
            pm_f2u_t a0{0.f, 0.f}, a1{0.f, 0.f};
            if (sig) pm_rows(sig, o0, o1, n_ext, pair, 7, s0, s1);
            if (att) pm_rows(att, o0, o1, n_ext, pair, 8, a0, a1);
            const double sl = fma(fv, s0.y - s0.x, s0.x), sh = fma(fv, s1.y - s1.x, s1.x);
            ss += fma(fu, sh - sl, sl);
            const float gu = (float)fu, gv = (float)fv;
            const float al = fmaf(gv, a0.y - a0.x, a0.x), ah = fmaf(gv, a1.y - a1.x, a1.x);
            as += fmaf(gu, ah - al, al);
        }
        const double l = moving ? P.hz * d / fabs(wz) : 0.0;
        const double q = (d + l * ss) * P.inv_cdt;
        const float amp = __expf(-(float)l * as) * __builtin_amdgcn_rcpf((float)d);
#pragma unroll
        for (int s = 0; s < R; ++s)
            if (s == r) { qc[s] = q; ac[s] = amp; }
    }

    float iz = P.inten_scale, pz_scale = P.pii_scale;                   // the voxel's own impedance
    if (inv2z && OLX_IN(v, P.vox, 12)) { iz = inv2z[v]; pz_scale = M.two_dt * iz; }

    const int s0 = lane * PM_SEG;
#pragma unroll
    for (int s = 0; s < PM_SEG; ++s) { re[s0 + s] = 0.f; im[s0 + s] = 0.f; }

    for (int f = 0; f < P.n_foci; ++f) {
        const double4* T = tab + (size_t)f * P.n_el;
        const float* W = wtab + (size_t)f * P.n_el;
        // 1. the voxel's window of samples, from the cache
        double umin = 1.0e300, umax = -1.0e300;
        for (int r = 0; r < nr; ++r) {
            const int e = lane + 64 * r;
            double q = 0.0;
#pragma unroll
            for (int s = 0; s < R; ++s) q = s == r ? qc[s] : q;
            if (e < P.n_el && W[e] != 0.f) {
                const double u = T[e].w + q;
                umin = fmin(umin, u); umax = fmax(umax, u);
            }
        }
        umin = pm_wave_mind(umin); umax = pm_wave_maxd(umax);
        const long long vf = (long long)f * P.vox + v;
        if (umin > umax) {                        // no driven element
            if constexpr (!TRACE) {
                if (lane == 0 && OLX_IN(vf, P.vox * P.n_foci, 6)) {
                    pmin_out[vf] = 0.f; if (pmax_out) pmax_out[vf] = 0.f; if (inten_out) inten_out[vf] = 0.f;
                    if constexpr (PII) pii_out[vf] = 0.f;
                }
            }
            continue;
        }
        const double lo = fmax(floor(umin) - 2.0, 0.0);
        const double hi = fmin(ceil(umax + P.tdt) + 2.0, (double)P.n_t);          // exclusive

        float pmax = 0.f, pmin = 0.f;             // (samples outside the window are 0: they bound both from the zero side)
        float e2 = 0.f;                           // PII: the lane's sum of p^2 over its samples of all passes
        float* const trace = pmin_out + ((long long)f * n_points + w) * P.n_t;       // TRACE: this (focus, point)'s row
        for (double base = lo; base < hi; base += PM_L) {
            double kbeg = 1.0e300, kend = -1.0e300;   // TRACE: first arrival, last burst end (the fp64 integers; the same in every pass)
            pm_lds_sync();
            // 2a. scatter the element terms into the difference array of this pass
            for (int r = 0; r < nr; ++r) {
                const int e = lane + 64 * r;
                double q = 0.0;
                float amp = 0.f;
#pragma unroll
                for (int s = 0; s < R; ++s) { q = s == r ? qc[s] : q; amp = s == r ? ac[s] : amp; }
                if (e >= P.n_el) continue;
                const float we = W[e];
                if (we == 0.f) continue;
                const double m = T[e].w;
                const double k0 = m + ceil(q), k1 = m + ceil(q + P.tdt);
                if constexpr (TRACE) { kbeg = fmin(kbeg, k0); kend = fmax(kend, k1); }
                if (k0 >= base + PM_L || k1 <= base || k1 <= k0) continue;      // after this pass, or over before it: nothing here
                double cyc = P.f0dt * ((m - lo) + q);
                cyc -= floor(cyc);
                const float ph = (float)cyc;
                const float a = we * amp;
                const float cr = a * __builtin_amdgcn_cosf(ph), ci = -a * __builtin_amdgcn_sinf(ph);
                const int i0 = k0 <= base ? 0 : (int)(k0 - base);
                if (OLX_IN(i0, PM_L, 0)) { atomicAdd(&re[i0], cr); atomicAdd(&im[i0], ci); }
                if (k1 < base + PM_L) {
                    const int i1 = (int)(k1 - base);
                    if (OLX_IN(i1, PM_L, 1)) { atomicAdd(&re[i1], -cr); atomicAdd(&im[i1], -ci); }
                }
            }
            pm_lds_sync();
            // 2b. prefix scan: the lane's own segment, then the exclusive scan of the segment totals across the wave
            float sr[PM_SEG], si[PM_SEG];
            float tr = 0.f, ti = 0.f;
#pragma unroll
            for (int s = 0; s < PM_SEG; ++s) {
                sr[s] = re[s0 + s]; si[s] = im[s0 + s];
                tr += sr[s]; ti += si[s];
                sr[s] = tr; si[s] = ti;
            }
            float cr = tr, ci = ti;                  // inclusive scan of the totals
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const float ur = __shfl_up(cr, o), ui = __shfl_up(ci, o);
                if (lane >= o) { cr += ur; ci += ui; }
            }
            cr -= tr; ci -= ti;                      // ... exclusive: the carry into this lane's segment
            pm_lds_sync();
#pragma unroll
            for (int s = 0; s < PM_SEG; ++s) { re[s0 + s] = 0.f; im[s0 + s] = 0.f; }     // (cleared for the next pass and the next focus)
            // 2c. p at the pass's samples: theta_k = 2 pi f0 dt (k - lo), exact at the segment's first sample, rotated by 2 pi f0 dt after it
            const double kfirst = base + s0;
            double cyc = P.f0dt * (kfirst - lo);
            cyc -= floor(cyc);
            float er = __builtin_amdgcn_cosf((float)cyc), ei = __builtin_amdgcn_sinf((float)cyc);
            const int nvalid = (int)fmin(fmax(hi - kfirst, 0.0), (double)PM_SEG);
            int sbeg = 0, send = nvalid;              // TRACE: the valid samples at which an element is or has been active
            if constexpr (TRACE) {
                kbeg = pm_wave_mind(kbeg); kend = pm_wave_maxd(kend);
                sbeg = (int)fmin(fmax(kbeg - kfirst, 0.0), (double)PM_SEG);
                send = min(nvalid, (int)fmin(fmax(kend - kfirst, 0.0), (double)PM_SEG));
            }
#pragma unroll
            for (int s = 0; s < PM_SEG; ++s) {
                const float p = er * (cr + sr[s]) - ei * (ci + si[s]);
                if constexpr (TRACE) {
                    if (s >= sbeg && s < send) {
                        const long long kk = (long long)kfirst + s;
                        if (OLX_IN(kk, P.n_t, 4)) trace[kk] = p;
                    }
                } else if (s < nvalid) {
                    pmax = fmaxf(pmax, p); pmin = fminf(pmin, p);
                    if constexpr (PII) e2 = fmaf(p, p, e2);
                }
                const float nr_ = er * P.rot_c - ei * P.rot_s;
                ei = fmaf(er, P.rot_s, ei * P.rot_c);
                er = nr_;
            }
        }
        if constexpr (!TRACE) {
            pmax = pm_wave_max(pmax); pmin = pm_wave_min(pmin);
            if constexpr (PII) e2 = pm_wave_sum(e2);
            if (lane == 0 && OLX_IN(vf, P.vox * P.n_foci, 2)) {
                const float pn = 0.f - pmin;          // (+0 where nothing arrived)
                pmin_out[vf] = pn;
                if (pmax_out) pmax_out[vf] = pmax;
                if (inten_out) inten_out[vf] = iz * pn * pn;
            }
            if constexpr (PII) {
                if (lane == 0 && OLX_IN(vf, P.vox * P.n_foci, 3)) pii_out[vf] = pz_scale * e2;
            }
        }
    }
}

OLX_BOUNDS_READER(pulsemed)

}  // namespace olx

using namespace olx;

static void launch_pm_table(olx_ctx* c) {
    const int fn = c->n_el * c->plan_foci;
    hipLaunchKernelGGL(pulse_med_table_k, dim3((fn + 255) / 256), dim3(256), 0, c->stream, c->d_pos, c->d_area, c->d_delays, c->d_apod, c->n_el,
                       c->plan_foci, c->pulse_plan_dt, c->p0_pa * c->freq / c->c, c->d_ptab, c->d_pw);      // (the dt of the plan, not of a later olx_field_pulse)
}

template <int R, bool PII, bool TRACE>
static void launch_pm(olx_ctx* c, dim3 grid, float* pm, float* px, float* it, float* pii, const long long* points, int n_points) {
    hipLaunchKernelGGL((field_pulse_med_k<R, PII, TRACE>), grid, dim3(64 * PM_WAVES), 0, c->stream, c->d_ptab, c->d_pw, c->d_pm_kb,
                       c->pm_has_sig ? (const double*)c->d_pm_sig : nullptr, c->pm_has_att ? (const float*)c->d_pm_att : nullptr, c->d_pm_plane_k,
                       c->d_pm_plane_of_k, c->pm_has_z ? (const float*)c->d_pm_inv2z : nullptr, c->pm, pm, px, it, pii, points, n_points);
}

void olx_launch_pulse_med(olx_ctx* c, float* pm) {
    const PulseParams& P = c->pm.P;
    launch_pm_table(c);
    const dim3 grid((unsigned)((P.vox + PM_WAVES - 1) / PM_WAVES));
    float* const px = (c->flags & OLX_OUT_PMAX) ? (float*)c->d_pmax : nullptr;
    float* const it = (c->flags & OLX_OUT_INTENSITY) ? (float*)c->d_inten : nullptr;
    const bool pii = (c->flags & OLX_OUT_PII) != 0;
    if (c->pulse_med_R == 4) {
        if (pii) launch_pm<4, true, false>(c, grid, pm, px, it, c->d_pii, nullptr, 0);
        else     launch_pm<4, false, false>(c, grid, pm, px, it, nullptr, nullptr, 0);
    } else {
        if (pii) launch_pm<16, true, false>(c, grid, pm, px, it, c->d_pii, nullptr, 0);
        else     launch_pm<16, false, false>(c, grid, pm, px, it, nullptr, nullptr, 0);
    }
}

void olx_launch_pulse_med_trace(olx_ctx* c, int n_points) {
    launch_pm_table(c);      // (the caller has zeroed c->d_ptrace on the stream)
    const dim3 grid((unsigned)((n_points + PM_WAVES - 1) / PM_WAVES));
    if (c->pulse_med_R == 4) launch_pm<4, false, true>(c, grid, c->d_ptrace, nullptr, nullptr, nullptr, c->d_ptrace_vox, n_points);
    else                     launch_pm<16, false, true>(c, grid, c->d_ptrace, nullptr, nullptr, nullptr, c->d_ptrace_vox, n_points);
}
