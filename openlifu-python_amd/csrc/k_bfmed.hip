// kernels 1m and 1a (bf_med_k<SIG, ATT>): the straight-ray walk of the beamformer through the media of olx_bf_set_medium (sigma -> StraightRay
// delays, "1m", SIG) and olx_bf_set_attenuation (a -> MediumCompensated apodization, "1a", ATT).  gfx950 (CDNA4, wave64) only.  Definitions:
// DESIGN.md section 2 ("StraightRay", "MediumCompensated"), fp64 oracles tests/medium_delay_oracle.py and tests/medium_apod_oracle.py.
//
// Per focus r_f and element e (fp64), g_e, d = |r_f - g_e| and tof = d / c exactly as bf_solve_k forms them (same expressions), dz = z_f - z_e:
//     E = 0 if dz == 0, else  l (sig~(r_f) / 2 + sum_k sig_k(crossing_k)),   l = hz max(d, dmin) / |dz|        A = the same sum over a [Np/m]
//     tau = tof + E / c,  delays = max_e tau - tau                                                             (SIG)
//     h = exp(-A) [S_e / max(d, dmin) with spreading],  apod = b (min_active h / h)  or  b (h / max_active h)  (ATT; b = kernel 1's, active: b > 0)
// k runs over the held (non-trivial) planes with t = (z_k - z_e) / dz strictly inside (0, 1) and z_k farther than ztol from z_f; sig_k is the
// bilinear, border-extended sample of plane k where the ray crosses it (oracle/field_oracle.c bilinear2), sig~ the trilinear, border-extended
// sample at the focus (a plane that is not held is zero).  Work map: one block per focus (all foci in one launch), lanes over elements, each lane
// walks the held planes; the block reduces max tau as kernel 1 does, and min / max h over the active lanes.  bf_solve_k runs first on the same
// table: its apodization is what SIG alone leaves there and what ATT reads as b.  SIG && ATT is ONE walk over the planes held by either volume
// (walk[p] = its plane in each, -1 = not held there): the crossing, its corner offsets and weights are formed once and applied to both.
#include "k_types.hip.h"
#include "olx_ctx.h"

namespace olx {

__device__ __forceinline__ double bfm_wave_max(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ double bfm_wave_min(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off, 64));
    return v;
}

// where fractional indices (u, v) fall in an [nx][ny] plane, clamped to the edge like the oracle's bilinear2: corner offsets and weights
struct BfmTap { long long o00, o01, o10, o11; double fu, fv; };
__device__ __forceinline__ BfmTap bfm_tap(int nx, int ny, double u, double v) {
    u = u < 0 ? 0 : (u > nx - 1 ? nx - 1 : u);
    v = v < 0 ? 0 : (v > ny - 1 ? ny - 1 : v);
    int i0 = (int)floor(u), j0 = (int)floor(v);
    if (i0 > nx - 2) i0 = nx - 2 < 0 ? 0 : nx - 2;
    if (j0 > ny - 2) j0 = ny - 2 < 0 ? 0 : ny - 2;
    const int i1 = i0 + 1 < nx ? i0 + 1 : i0, j1 = j0 + 1 < ny ? j0 + 1 : j0;
    return {(long long)i0 * ny + j0, (long long)i0 * ny + j1, (long long)i1 * ny + j0, (long long)i1 * ny + j1, u - i0, v - j0};
}
// bilinear sample of the plane at offset plane_off of s (n_ext doubles in all) at a tap
__device__ __forceinline__ double bfm_sample(const double* __restrict__ s, long long plane_off, long long n_ext, const BfmTap& T, int site) {
    const long long o00 = plane_off + T.o00, o01 = plane_off + T.o01, o10 = plane_off + T.o10, o11 = plane_off + T.o11;
    const double s00 = OLX_IN(o00, n_ext, site) ? s[o00] : 0.0, s01 = OLX_IN(o01, n_ext, site) ? s[o01] : 0.0;
    const double s10 = OLX_IN(o10, n_ext, site) ? s[o10] : 0.0, s11 = OLX_IN(o11, n_ext, site) ? s[o11] : 0.0;
    return (1 - T.fu) * ((1 - T.fv) * s00 + T.fv * s01) + T.fu * ((1 - T.fv) * s10 + T.fv * s11);
}
// the focus' own half layer of one volume: trilinear, border-extended (uniform over the block); pk[k] = held plane of grid plane k, -1 = zero there
__device__ __forceinline__ double bfm_focus_sample(const double* __restrict__ s, const int* __restrict__ pk, int n_held, const BfMedParams& P,
                                                   double fx, double fy, double fz, int site) {
    if (n_held <= 0) return 0.0;
    const long long nxy = (long long)P.nx * P.ny, n_ext = nxy * n_held;
    const BfmTap T = bfm_tap(P.nx, P.ny, (fx - P.ox) / P.hx, (fy - P.oy) / P.hy);
    double w = (fz - P.oz) / P.hz;
    w = w < 0 ? 0 : (w > P.nz - 1 ? P.nz - 1 : w);
    int k0 = (int)floor(w);
    if (k0 > P.nz - 2) k0 = P.nz - 2 < 0 ? 0 : P.nz - 2;
    const int k1 = k0 + 1 < P.nz ? k0 + 1 : k0;
    const double fw = w - k0;
    const int p0 = OLX_IN(k0, P.nz, site + 1) ? pk[k0] : -1, p1 = OLX_IN(k1, P.nz, site + 1) ? pk[k1] : -1;
    const double s0 = p0 >= 0 ? bfm_sample(s, p0 * nxy, n_ext, T, site) : 0.0;
    const double s1 = p1 >= 0 ? bfm_sample(s, p1 * nxy, n_ext, T, site) : 0.0;
    return (1 - fw) * s0 + fw * s1;
}

// bounds sites of the debug library: 0 sigma texels, 1 sigma plane map, 2 attenuation texels, 3 attenuation plane map, 4 the walk's plane pairs
template <bool SIG, bool ATT>
__global__ __launch_bounds__(BF_THREADS) void bf_med_k(
    const double* __restrict__ pos,  // [3][N]
    int n, const double* __restrict__ foci /*[F][3]*/, const double* __restrict__ M /*[16]*/, const BfMedParams P /*n_planes: the walked planes*/,
    const double* __restrict__ sig /*[n_sig][nx][ny]*/, const int* __restrict__ sig_pk /*[nz], -1 = not held*/, int n_sig,
    const double* __restrict__ att /*[n_att][nx][ny] Np/m*/, const int* __restrict__ att_pk /*[nz]*/, int n_att,
    const double* __restrict__ zp /*[n_planes] z of the walked planes*/, const int2* __restrict__ walk /*[n_planes] (sigma, a) plane; SIG && ATT only*/,
    const double* __restrict__ area /*[N]*/, int mode, int spreading,
    double* __restrict__ delays /*[F][N]*/, double* __restrict__ apod /*[F][N]*/, double* __restrict__ hbuf /*[F][N] scratch*/) {
    __shared__ double s_focus[3];
    __shared__ double s_M[16];
    __shared__ double s_red[3][BF_THREADS / 64];
    const int f = blockIdx.x, tid = threadIdx.x;
    if (tid < 3) s_focus[tid] = foci[3 * f + tid];
    if (tid >= 64 && tid < 80) s_M[tid - 64] = M[tid - 64];
    __syncthreads();
    const double fx = s_focus[0], fy = s_focus[1], fz = s_focus[2];
    const long long nxy = (long long)P.nx * P.ny;
    double sf = 0.0, af = 0.0;
    if constexpr (SIG) sf = bfm_focus_sample(sig, sig_pk, n_sig, P, fx, fy, fz, 0);
    if constexpr (ATT) af = bfm_focus_sample(att, att_pk, n_att, P, fx, fy, fz, 2);
    double* dl = delays + (size_t)f * n;
    double* ap = apod + (size_t)f * n;
    double* hb = hbuf + (size_t)f * n;
    double lmax = -1.0, hmin = INFINITY, hmax = -INFINITY;
    for (int e = tid; e < n; e += BF_THREADS) {
        const double px = pos[e], py = pos[n + e], pz = pos[2 * n + e];
        // gpos = (M . [p,1])[:3], d and tof: bf_solve_k's expressions (a medium with sig == 0 gives its delays bit for bit)
        const double gx = s_M[0] * px + s_M[1] * py + s_M[2] * pz + s_M[3];
        const double gy = s_M[4] * px + s_M[5] * py + s_M[6] * pz + s_M[7];
        const double gz = s_M[8] * px + s_M[9] * py + s_M[10] * pz + s_M[11];
        const double vx = fx - gx, vy = fy - gy, vz = fz - gz;
        const double d = sqrt(vx * vx + vy * vy + vz * vz);
        double E = 0.0, A = 0.0;
        if (vz != 0.0) {
            double ssum = 0.5 * sf, asum = 0.5 * af;
            for (int p = 0; p < P.n_planes; ++p) {
                const double zk = zp[p];
                const double t = (zk - gz) / vz;
                if (!(t > 0 && t < 1) || fabs(zk - fz) <= P.ztol) continue;
                const BfmTap T = bfm_tap(P.nx, P.ny, (gx + t * vx - P.ox) / P.hx, (gy + t * vy - P.oy) / P.hy);
                if constexpr (SIG && ATT) {
                    const int2 w = walk[p];
                    if (w.x >= 0 && OLX_IN(w.x, n_sig, 4)) ssum += bfm_sample(sig, w.x * nxy, nxy * n_sig, T, 0);
                    if (w.y >= 0 && OLX_IN(w.y, n_att, 4)) asum += bfm_sample(att, w.y * nxy, nxy * n_att, T, 2);
                } else if constexpr (SIG) {
                    ssum += bfm_sample(sig, p * nxy, nxy * n_sig, T, 0);
                } else {
                    asum += bfm_sample(att, p * nxy, nxy * n_att, T, 2);
                }
            }
            const double l = P.hz * fmax(d, P.dmin) / fabs(vz);
            E = l * ssum;
            A = l * asum;
        }
        if constexpr (SIG) {
            const double tof = d / P.c;
            const double tau = tof + E / P.c;
            dl[e] = tau;
            lmax = fmax(lmax, tau);
        }
        if constexpr (ATT) {
            double h = exp(-A);                     // A == 0 (no attenuation on the ray): exactly 1
            if (spreading) h = h * area[e] / fmax(d, P.dmin);
            hb[e] = h;
            if (ap[e] > 0) { hmin = fmin(hmin, h); hmax = fmax(hmax, h); }
        }
    }
    if constexpr (SIG) lmax = bfm_wave_max(lmax);
    if constexpr (ATT) { hmin = bfm_wave_min(hmin); hmax = bfm_wave_max(hmax); }
    if ((tid & 63) == 0) {
        if constexpr (SIG) s_red[0][tid >> 6] = lmax;
        if constexpr (ATT) { s_red[1][tid >> 6] = hmin; s_red[2][tid >> 6] = hmax; }
    }
    __syncthreads();
    if constexpr (SIG) {
        double bmax = s_red[0][0];
#pragma unroll
        for (int w = 1; w < BF_THREADS / 64; ++w) bmax = fmax(bmax, s_red[0][w]);
        for (int e = tid; e < n; e += BF_THREADS) dl[e] = bmax - dl[e];  // same thread wrote dl[e]
    }
    if constexpr (ATT) {
        double bmin = s_red[1][0], bmax = s_red[2][0];
#pragma unroll
        for (int w = 1; w < BF_THREADS / 64; ++w) { bmin = fmin(bmin, s_red[1][w]); bmax = fmax(bmax, s_red[2][w]); }
        for (int e = tid; e < n; e += BF_THREADS) {                      // same thread wrote hb[e]; a lane with b == 0 keeps it
            const double b = ap[e], h = hb[e];
            if (b > 0) ap[e] = b * (mode == OLX_COMP_MATCHED ? h / bmax : bmin / h);
        }
    }
}

OLX_BOUNDS_READER(bfmed)

}  // namespace olx

using namespace olx;

void olx_launch_bfmed(olx_ctx* c, int n_foci) {
    hipLaunchKernelGGL((bf_med_k<true, false>), dim3(n_foci), dim3(BF_THREADS), 0, c->stream, c->d_pos, c->n_el, c->d_foci, c->d_M, c->bm,
                       c->d_bm_sig, c->d_bm_pk, c->bm.n_planes, nullptr, nullptr, 0, c->d_bm_zp, nullptr, nullptr, 0, 0, c->d_delays, nullptr, nullptr);
}

// kernel 1a over the apodization column of the steering table, alone (the attenuation's own planes) or in one walk with kernel 1m's delays
// (the planes held by either volume: c->d_bc_zp / d_bc_walk, olx_bf_solve_compensated)
void olx_launch_bfapod(olx_ctx* c, int n_foci, int mode, int spreading, bool with_delays) {
    if (with_delays) {
        BfMedParams P = c->bm;
        P.n_planes = c->bc_planes;
        hipLaunchKernelGGL((bf_med_k<true, true>), dim3(n_foci), dim3(BF_THREADS), 0, c->stream, c->d_pos, c->n_el, c->d_foci, c->d_M, P,
                           c->d_bm_sig, c->d_bm_pk, c->bm.n_planes, c->d_ba_att, c->d_ba_pk, c->ba.n_planes, c->d_bc_zp, c->d_bc_walk, c->d_area,
                           mode, spreading, c->d_delays, c->d_apod, c->d_ba_h);
    } else {
        hipLaunchKernelGGL((bf_med_k<false, true>), dim3(n_foci), dim3(BF_THREADS), 0, c->stream, c->d_pos, c->n_el, c->d_foci, c->d_M, c->ba,
                           nullptr, nullptr, 0, c->d_ba_att, c->d_ba_pk, c->ba.n_planes, c->d_ba_zp, nullptr, c->d_area,
                           mode, spreading, nullptr, c->d_apod, c->d_ba_h);
    }
}
