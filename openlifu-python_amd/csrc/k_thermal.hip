// kernel 3 (thermal_pack_k, thermal_step_k): Pennes bioheat rise over a pulse sequence, explicit FTCS on the simulation grid.
// gfx950 (CDNA4, wave64) only.  Definition: DESIGN.md section 2 ("thermal model") and section 5.8, fp64 oracle tests/thermal_oracle.py.
//
// State: the rise dT above the baseline (fp32; never the absolute temperature, ulp(37) ~ 30 ulp(1)).  One step, voxel v (C order, z fastest):
//     acc   = sum over the six faces of K_face (dT_nb - dT_v) - W dT_v        (dT_nb = 0 one spacing outside the grid)
//     dT'_v = dT_v + dt / (rho Cp)_v acc + s_v sum_f tau_{n,f} I_f(v)        s_v = 2 alpha_v 1e4 / (rho Cp)_v
// K_face = harmonic mean of the two voxels' kappa / h^2 inside, kappa_v / h^2 on a boundary face.  The coefficient volumes hold each voxel's
// three "+" faces (its "-" faces are its lower neighbours' "+" faces; on the high boundary the "+" face is the boundary face) and a sink
// term = W + the conductances of its low boundary faces, so that acc = sum_+ K+ (dT_nb - dT) + sum_- K- (dT_nb - dT) - sink dT.
// A uniform medium streams no coefficient volume (UNI): K = kappa / h^2 per axis, and the low boundary faces are added from the indices.
// After the step: rise_max = max(rise_max, dT'), cem += dt / 60 R^(43 - T), T = T_b + dT', R = 0.5 (T >= 43) or 0.25.
// The source of step n reads I_f only for the foci of the schedule's row n (CSR on the host: the launch gets the row's offset and length).
// Trace points: the launch of step n writes the state after step n - 1 (its input) at every point; thermal_trace_k writes the last row.
#include "k_types.hip.h"
#include "olx_ctx.h"
#include "olx_launch.h"

namespace olx {

constexpr int THERMAL_BLOCK = 256;

__device__ __forceinline__ float harm_mean(float a, float b) { return 2.0f * a * b / (a + b); }

// per-voxel coefficients of a heterogeneous medium (NULL volume = the scalar of ThermalParams) and the largest FTCS rate
// max_v (sum_faces K + W) / (rho Cp)_v (positive floats: their bit patterns order as unsigned integers)
__global__ __launch_bounds__(THERMAL_BLOCK) void thermal_pack_k(const float* __restrict__ rho, const float* __restrict__ cp, const float* __restrict__ kap,
                                                                const float* __restrict__ alpha, const ThermalParams P, float4* __restrict__ coef,
                                                                float* __restrict__ irc, float* __restrict__ sfac, unsigned* __restrict__ rate_max) {
    const long long v = (long long)blockIdx.x * THERMAL_BLOCK + threadIdx.x;
    float rate = 0.f;
    if (v < P.vox) {
        const long long pl = (long long)P.ny * P.nz;
        const int i = (int)(v / pl), j = (int)((v % pl) / P.nz), k = (int)(v % P.nz);
        auto kv = [&](long long u) { return kap ? kap[u] : P.kappa0; };
        const float kc = kv(v);
        const float rc = (rho ? rho[v] : P.rho0) * (cp ? cp[v] : P.cp0);
        const float gxp = (i + 1 < P.nx ? harm_mean(kc, kv(v + pl)) : kc) * P.ihx2;
        const float gyp = (j + 1 < P.ny ? harm_mean(kc, kv(v + P.nz)) : kc) * P.ihy2;
        const float gzp = (k + 1 < P.nz ? harm_mean(kc, kv(v + 1)) : kc) * P.ihz2;
        const float gxm = (i > 0 ? harm_mean(kc, kv(v - pl)) : kc) * P.ihx2;
        const float gym = (j > 0 ? harm_mean(kc, kv(v - P.nz)) : kc) * P.ihy2;
        const float gzm = (k > 0 ? harm_mean(kc, kv(v - 1)) : kc) * P.ihz2;
        const float sink = P.perf + (i == 0 ? gxm : 0.f) + (j == 0 ? gym : 0.f) + (k == 0 ? gzm : 0.f);
        if (OLX_IN(v, P.vox, 0)) {
            coef[v] = make_float4(gxp, gyp, gzp, sink);
            irc[v] = 1.0f / rc;
            sfac[v] = 2.0f * (alpha ? alpha[v] : P.alpha0) * 1e4f / rc;
        }
        rate = (gxp + gyp + gzp + gxm + gym + gzm + P.perf) / rc;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) rate = fmaxf(rate, __shfl_xor(rate, o));
    if ((threadIdx.x & 63) == 0) atomicMax(rate_max, __float_as_uint(rate));
}

template <bool UNI>
__global__ __launch_bounds__(THERMAL_BLOCK) void thermal_step_k(const float* __restrict__ tin, float* __restrict__ tout, float* __restrict__ rmax,
                                                                float* __restrict__ cem, const float4* __restrict__ coef, const float* __restrict__ irc,
                                                                const float* __restrict__ sfac, const float* __restrict__ inten,
                                                                const int* __restrict__ s_focus, const float* __restrict__ s_tau, int e0, int ne,
                                                                const ThermalParams P, const ThermalStep S, const long long* __restrict__ pts,
                                                                float* __restrict__ trace_prev) {
    const long long v = (long long)blockIdx.x * THERMAL_BLOCK + threadIdx.x;
    if (trace_prev && blockIdx.x == 0)          // the state after the previous step at the trace points (this launch's input)
        for (int p = threadIdx.x; p < S.npts; p += THERMAL_BLOCK)
            if (OLX_IN(pts[p], P.vox, 1)) trace_prev[p] = tin[pts[p]];
    if (v >= P.vox) return;
    const long long pl = (long long)P.ny * P.nz;
    const int i = (int)(v / pl), j = (int)((v % pl) / P.nz), k = (int)(v % P.nz);
    const float t = tin[v];
    float gxp, gyp, gzp, sink, gxm, gym, gzm, a, s;
    if (UNI) {
        gxp = gxm = P.gx; gyp = gym = P.gy; gzp = gzm = P.gz;
        sink = P.perf + (i == 0 ? P.gx : 0.f) + (j == 0 ? P.gy : 0.f) + (k == 0 ? P.gz : 0.f);
        a = P.irc0; s = P.sfac0;
    } else {
        const float4 c = coef[v];
        gxp = c.x; gyp = c.y; gzp = c.z; sink = c.w;
        gxm = i > 0 ? coef[v - pl].x : 0.f;
        gym = j > 0 ? coef[v - P.nz].y : 0.f;
        gzm = k > 0 ? coef[v - 1].z : 0.f;
        a = irc[v]; s = 0.f;
    }
    float acc = gxp * ((i + 1 < P.nx ? tin[v + pl] : 0.f) - t) + gyp * ((j + 1 < P.ny ? tin[v + P.nz] : 0.f) - t)
              + gzp * ((k + 1 < P.nz ? tin[v + 1] : 0.f) - t);
    if (i > 0) acc += gxm * (tin[v - pl] - t);
    if (j > 0) acc += gym * (tin[v - P.nz] - t);
    if (k > 0) acc += gzm * (tin[v - 1] - t);
    acc -= sink * t;
    float q = 0.f;                               // sum_f tau_{n,f} I_f(v) of this step's schedule row (wave-uniform loop)
    for (int e = e0; e < e0 + ne; ++e) {
        const int f = s_focus[e];
        const long long u = (long long)f * P.vox + v;
        if (OLX_IN(u, P.vox * S.n_foci, 2)) q = fmaf(s_tau[e], inten[u], q);
    }
    if (ne > 0 && !UNI) s = sfac[v];
    const float tn = fmaf(S.dt * a, acc, t) + s * q;
    tout[v] = tn;
    rmax[v] = fmaxf(rmax[v], tn);
    const float x = S.tb43 + tn;                 // T - 43
    cem[v] += S.dt_min * exp2f(x >= 0.f ? x : 2.0f * x);
}

// the trace row of the last step of a run: the state it left
__global__ void thermal_trace_k(const float* __restrict__ t, const long long* __restrict__ pts, int npts, long long vox, float* __restrict__ row) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < npts && OLX_IN(pts[p], vox, 3)) row[p] = t[pts[p]];
}

OLX_BOUNDS_READER(thermal)

}  // namespace olx

using namespace olx;

void olx_thermal_pack(olx_ctx* c, const float* rho, const float* cp, const float* kap, const float* alpha) {
    const ThermalParams& P = c->th;
    hipLaunchKernelGGL(thermal_pack_k, dim3((unsigned)((P.vox + THERMAL_BLOCK - 1) / THERMAL_BLOCK)), dim3(THERMAL_BLOCK), 0, c->stream,
                       rho, cp, kap, alpha, P, c->d_th_coef, c->d_th_irc, c->d_th_sfac, c->d_th_rate);
}

void olx_thermal_step(olx_ctx* c, const float* inten, int step, const ThermalStep& S) {
    const ThermalParams& P = c->th;
    const int e0 = c->th_row[step], ne = c->th_row[step + 1] - e0;
    const float* tin = c->d_th_T[c->th_cur];
    float* tout = c->d_th_T[c->th_cur ^ 1];
    float* trace_prev = (S.npts > 0 && step > 0) ? c->d_th_trace + (size_t)(step - 1) * S.npts : nullptr;
    const dim3 grid((unsigned)((P.vox + THERMAL_BLOCK - 1) / THERMAL_BLOCK));
    if (c->th_uniform)
        hipLaunchKernelGGL(thermal_step_k<true>, grid, dim3(THERMAL_BLOCK), 0, c->stream, tin, tout, c->d_th_max, c->d_th_cem, nullptr, nullptr, nullptr,
                           inten, c->d_th_sf, c->d_th_tau, e0, ne, P, S, c->d_th_pts, trace_prev);
    else
        hipLaunchKernelGGL(thermal_step_k<false>, grid, dim3(THERMAL_BLOCK), 0, c->stream, tin, tout, c->d_th_max, c->d_th_cem, c->d_th_coef, c->d_th_irc,
                           c->d_th_sfac, inten, c->d_th_sf, c->d_th_tau, e0, ne, P, S, c->d_th_pts, trace_prev);
    c->th_cur ^= 1;
}

void olx_thermal_trace_last(olx_ctx* c, int step) {
    const int np = c->th_npts;
    if (np <= 0) return;
    hipLaunchKernelGGL(thermal_trace_k, dim3((np + 255) / 256), dim3(256), 0, c->stream, c->d_th_T[c->th_cur], c->d_th_pts, np, c->th.vox,
                       c->d_th_trace + (size_t)step * np);
}
