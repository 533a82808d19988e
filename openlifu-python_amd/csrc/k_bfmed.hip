// kernel 1m (bf_med_k): StraightRay delays -- kernel 1's geometric time of flight plus the straight-ray extra path E through the medium of
// olx_bf_set_medium.  gfx950 (CDNA4, wave64) only.  Definition: DESIGN.md section 2 ("StraightRay"), fp64 oracle tests/medium_delay_oracle.py.
//
// Per focus r_f and element e (fp64), g_e, d = |r_f - g_e| and tof = d / c exactly as bf_solve_k forms them (same expressions), dz = z_f - z_e:
//     E = 0 if dz == 0, else  l (sig~(r_f) / 2 + sum_k sig_k(crossing_k)),   l = hz max(d, dmin) / |dz|
//     tau = tof + E / c,  delays = max_e tau - tau
// k runs over the held (non-trivial) planes with t = (z_k - z_e) / dz strictly inside (0, 1) and z_k farther than ztol from z_f; sig_k is the
// bilinear, border-extended sample of plane k where the ray crosses it (oracle/field_oracle.c bilinear2), sig~ the trilinear, border-extended
// sample at the focus (a plane that is not held is zero).  Work map: one block per focus (all foci in one launch), lanes over elements, each lane
// walks the held planes; the block reduces max tau as kernel 1 does.  The apodization is kernel 1's (bf_solve_k runs first on the same table).
#include "k_types.hip.h"
#include "olx_ctx.h"

namespace olx {

__device__ __forceinline__ double bfm_wave_max(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    return v;
}

// bilinear sample of one [nx][ny] plane (offset plane_off into sig) at fractional indices (u, v), clamped to the edge like the oracle's bilinear2
__device__ __forceinline__ double bfm_bilinear(const double* __restrict__ s, long long plane_off, long long n_sig, int nx, int ny, double u, double v) {
    u = u < 0 ? 0 : (u > nx - 1 ? nx - 1 : u);
    v = v < 0 ? 0 : (v > ny - 1 ? ny - 1 : v);
    int i0 = (int)floor(u), j0 = (int)floor(v);
    if (i0 > nx - 2) i0 = nx - 2 < 0 ? 0 : nx - 2;
    if (j0 > ny - 2) j0 = ny - 2 < 0 ? 0 : ny - 2;
    const int i1 = i0 + 1 < nx ? i0 + 1 : i0, j1 = j0 + 1 < ny ? j0 + 1 : j0;
    const double fu = u - i0, fv = v - j0;
    const long long o00 = plane_off + (long long)i0 * ny + j0, o01 = plane_off + (long long)i0 * ny + j1;
    const long long o10 = plane_off + (long long)i1 * ny + j0, o11 = plane_off + (long long)i1 * ny + j1;
    const double s00 = OLX_IN(o00, n_sig, 0) ? s[o00] : 0.0, s01 = OLX_IN(o01, n_sig, 0) ? s[o01] : 0.0;
    const double s10 = OLX_IN(o10, n_sig, 0) ? s[o10] : 0.0, s11 = OLX_IN(o11, n_sig, 0) ? s[o11] : 0.0;
    return (1 - fu) * ((1 - fv) * s00 + fv * s01) + fu * ((1 - fv) * s10 + fv * s11);
}

__global__ __launch_bounds__(BF_THREADS) void bf_med_k(
    const double* __restrict__ pos,  // [3][N]
    int n, const double* __restrict__ foci /*[F][3]*/, const double* __restrict__ M /*[16]*/, const BfMedParams P,
    const double* __restrict__ sig /*[n_planes][nx][ny]*/, const double* __restrict__ zp /*[n_planes]*/,
    const int* __restrict__ plane_of_k /*[nz], -1 = not held*/, double* __restrict__ delays /*[F][N]*/) {
    __shared__ double s_focus[3];
    __shared__ double s_M[16];
    __shared__ double s_red[BF_THREADS / 64];
    const int f = blockIdx.x, tid = threadIdx.x;
    if (tid < 3) s_focus[tid] = foci[3 * f + tid];
    if (tid >= 64 && tid < 80) s_M[tid - 64] = M[tid - 64];
    __syncthreads();
    const double fx = s_focus[0], fy = s_focus[1], fz = s_focus[2];
    const long long nxy = (long long)P.nx * P.ny, n_sig = nxy * P.n_planes;
    // the focus' own half layer: trilinear, border-extended (uniform over the block)
    double sf = 0.0;
    if (P.n_planes > 0) {
        const double u = (fx - P.ox) / P.hx, v = (fy - P.oy) / P.hy;
        double w = (fz - P.oz) / P.hz;
        w = w < 0 ? 0 : (w > P.nz - 1 ? P.nz - 1 : w);
        int k0 = (int)floor(w);
        if (k0 > P.nz - 2) k0 = P.nz - 2 < 0 ? 0 : P.nz - 2;
        const int k1 = k0 + 1 < P.nz ? k0 + 1 : k0;
        const double fw = w - k0;
        const int p0 = OLX_IN(k0, P.nz, 1) ? plane_of_k[k0] : -1, p1 = OLX_IN(k1, P.nz, 1) ? plane_of_k[k1] : -1;
        const double s0 = p0 >= 0 ? bfm_bilinear(sig, p0 * nxy, n_sig, P.nx, P.ny, u, v) : 0.0;
        const double s1 = p1 >= 0 ? bfm_bilinear(sig, p1 * nxy, n_sig, P.nx, P.ny, u, v) : 0.0;
        sf = (1 - fw) * s0 + fw * s1;
    }
    double* dl = delays + (size_t)f * n;
    double lmax = -1.0;
    for (int e = tid; e < n; e += BF_THREADS) {
        const double px = pos[e], py = pos[n + e], pz = pos[2 * n + e];
        // gpos = (M . [p,1])[:3], d and tof: bf_solve_k's expressions (a medium with sig == 0 gives its delays bit for bit)
        const double gx = s_M[0] * px + s_M[1] * py + s_M[2] * pz + s_M[3];
        const double gy = s_M[4] * px + s_M[5] * py + s_M[6] * pz + s_M[7];
        const double gz = s_M[8] * px + s_M[9] * py + s_M[10] * pz + s_M[11];
        const double vx = fx - gx, vy = fy - gy, vz = fz - gz;
        const double d = sqrt(vx * vx + vy * vy + vz * vz);
        const double tof = d / P.c;
        double E = 0.0;
        if (vz != 0.0) {
            double ssum = 0.5 * sf;
            for (int p = 0; p < P.n_planes; ++p) {
                const double zk = zp[p];
                const double t = (zk - gz) / vz;
                if (!(t > 0 && t < 1) || fabs(zk - fz) <= P.ztol) continue;
                ssum += bfm_bilinear(sig, p * nxy, n_sig, P.nx, P.ny, (gx + t * vx - P.ox) / P.hx, (gy + t * vy - P.oy) / P.hy);
            }
            E = P.hz * fmax(d, P.dmin) / fabs(vz) * ssum;
        }
        const double tau = tof + E / P.c;
        dl[e] = tau;
        lmax = fmax(lmax, tau);
    }
    lmax = bfm_wave_max(lmax);
    if ((tid & 63) == 0) s_red[tid >> 6] = lmax;
    __syncthreads();
    double bmax = s_red[0];
#pragma unroll
    for (int w = 1; w < BF_THREADS / 64; ++w) bmax = fmax(bmax, s_red[w]);
    for (int e = tid; e < n; e += BF_THREADS) dl[e] = bmax - dl[e];  // same thread wrote dl[e]
}

OLX_BOUNDS_READER(bfmed)

}  // namespace olx

using namespace olx;

void olx_launch_bfmed(olx_ctx* c, int n_foci) {
    hipLaunchKernelGGL(bf_med_k, dim3(n_foci), dim3(BF_THREADS), 0, c->stream, c->d_pos, c->n_el, c->d_foci, c->d_M, c->bm,
                       c->d_bm_sig, c->d_bm_zp, c->d_bm_pk, c->d_delays);
}
