// kernel 4 (steer_table_k, steer_map_k): the steering map -- focal pressure when the array is steered to each voxel.
// gfx950 (CDNA4, wave64) only.  Definition: DESIGN.md section 2 ("Steering map"), fp64 oracle tests/steering_oracle.py.
//
// Per candidate voxel v at r_v = origin + index spacing and element e (position g_e, unit normal n_e, area S_e), in the array frame:
//     w = r_v - g_e,  d = |w|,  d' = max(d, dmin),  dmin = min(spacing) / 2
//     s = |w x n_e| / d (0 at d = 0),  theta = arcsin(min(s, 1))                                  kernel 1's folded angle
//     a_e = Uniform: value | MaxAngle: 1[theta <= theta_max] | PiecewiseLinear: clip((zero - theta) / (zero - rolloff), 0, 1)
//     P(v) = (P0 / lambda) sum_e a_e S_e D_e(v) exp(-alpha d') / d'   [Pa],   n_active(v) = #{ e : a_e > 0 }
// D_e = the piston factor of kernel 2a-d (opt-in), alpha a uniform absorption [Np/m].  P(v) is the CW field of kernel 2 at v when the
// array is steered to v with Direct delays and this apodization: every term arrives in phase, so no sin / cos is left.
//
// Precision: w is formed in fp64 (voxel coordinate from the integer index, minus the fp64 element position) and rounded ONCE to fp32.
// The decision of MaxAngle -- and the a_e > 0 decision of PiecewiseLinear, theta < zero, which n_active counts -- is made in fp64 without
// an arcsin: |w x n|^2 <= (<) sin^2(limit) |w|^2, sin^2 from the host; a limit >= 90 deg passes everything (lim2 = 2).  A flipped decision
// would move a whole term, ~1/N of the value (the argument of the pulsed kernel's activity rule).  Everything else is fp32, including
// PiecewiseLinear's asinf.
//
// Work map as kernel 2a: rows of nz voxels, a lane owns 4 consecutive z voxels, so the x / y parts of w, of the cross product and of the
// direction cosines are formed once per (lane, element).  The element records are wave-uniform and arrive through the scalar cache.
// One 16-byte store of P and one of n_active per lane; the last partial quad of a row dword by dword.  No LDS.
#include "k_types.hip.h"
#include "olx_ctx.h"
#include "olx_launch.h"

namespace olx {

typedef int intx4u_t __attribute__((ext_vector_type(4), aligned(4)));

enum { STEER_UNIFORM = 0, STEER_MAXANGLE = 1, STEER_PIECEWISE = 2 };

// one thread per element: the fp64 and fp32 records (olx_params.h, STEER_TD / STEER_TF).  ap = { xaxis [N][3], size_m [N][2] } or null.
__global__ __launch_bounds__(256) void steer_table_k(const double* __restrict__ pos, const double* __restrict__ nrm, const double* __restrict__ area,
                                                     const double* __restrict__ ap, int n, double wscale /* P0 / lambda */, double inv_2lambda,
                                                     double* __restrict__ tabd, float* __restrict__ tabf) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    double nx = nrm[e], ny = nrm[n + e], nz = nrm[2 * n + e];
    const double nn = sqrt(nx * nx + ny * ny + nz * nz);
    nx /= nn; ny /= nn; nz /= nn;
    double* td = tabd + (size_t)e * STEER_TD;
    float* tf = tabf + (size_t)e * STEER_TF;
    td[0] = pos[e]; td[1] = pos[n + e]; td[2] = pos[2 * n + e]; td[3] = 0.0;
    td[4] = nx; td[5] = ny; td[6] = nz; td[7] = 0.0;
    tf[0] = (float)nx; tf[1] = (float)ny; tf[2] = (float)nz; tf[3] = (float)(area[e] * wscale);
#pragma unroll
    for (int k = 4; k < STEER_TF; ++k) tf[k] = 0.f;
    if (ap) {
        const double ex = ap[3 * e], ey = ap[3 * e + 1], ez = ap[3 * e + 2];
        tf[4] = (float)ex; tf[5] = (float)ey; tf[6] = (float)ez; tf[7] = (float)(ap[3 * (size_t)n + 2 * e] * inv_2lambda);
        tf[8] = (float)(ny * ez - nz * ey); tf[9] = (float)(nz * ex - nx * ez); tf[10] = (float)(nx * ey - ny * ex);      // ey = n x ex
        tf[11] = (float)(ap[3 * (size_t)n + 2 * e + 1] * inv_2lambda);
    }
}

template <int KIND, bool DIRECTIVITY, bool ABSORB>
__global__ __launch_bounds__(FIELD_THREADS) void steer_map_k(const double* __restrict__ tabd, const float* __restrict__ tabf,
                                                             float* __restrict__ pfocal, int* __restrict__ nact, const SteerParams P) {
    constexpr int ZPL = 4;
    const int cpr = (P.nz + ZPL - 1) / ZPL;  // chunks per row
    const long long lane_id = (long long)blockIdx.x * FIELD_THREADS + threadIdx.x;
    const long long rows = (long long)P.nx * P.ny;
    const long long row = lane_id / cpr;
    if (row >= rows) return;
    const int chunk = (int)(lane_id - row * cpr);
    const int i = (int)(row / P.ny), j = (int)(row - (long long)i * P.ny);
    const int k0 = chunk * ZPL;
    const double xv = P.ox + i * P.hx, yv = P.oy + j * P.hy;
    double zv[ZPL];
    float acc[ZPL];
    int cnt[ZPL];
#pragma unroll
    for (int q = 0; q < ZPL; ++q) { zv[q] = P.oz + (k0 + q) * P.hz; acc[q] = 0.f; cnt[q] = 0; }
    for (int e = 0; e < P.n_el; ++e) {
        const double* td = tabd + (size_t)e * STEER_TD;
        const float* tf = tabf + (size_t)e * STEER_TF;
        const double wxd = xv - td[0], wyd = yv - td[1], gz = td[2];
        const float wx = (float)wxd, wy = (float)wyd;
        const float r2 = fmaf(wy, wy, wx * wx);
        const float amp = tf[3];
        // the parts of w x n, |w|^2 and w . ex, w . ey that do not depend on z
        double ndx = 0, ndy = 0, cx0d = 0, cy0d = 0, cz2d = 0, r2d = 0;
        if constexpr (KIND != STEER_UNIFORM) {
            ndx = td[4]; ndy = td[5];
            const double ndz = td[6], czd = wxd * ndy - wyd * ndx;
            cx0d = wyd * ndz; cy0d = -wxd * ndz; cz2d = czd * czd;
            r2d = fma(wyd, wyd, wxd * wxd);
        }
        float nfx = 0, nfy = 0, cx0 = 0, cy0 = 0, cz2 = 0;
        if constexpr (KIND == STEER_PIECEWISE) {
            nfx = tf[0]; nfy = tf[1];
            const float nfz = tf[2], cz = fmaf(wx, nfy, -wy * nfx);
            cx0 = wy * nfz; cy0 = -wx * nfz; cz2 = cz * cz;
        }
        float px = 0, py = 0;
        if constexpr (DIRECTIVITY) { px = fmaf(wy, tf[5], wx * tf[4]); py = fmaf(wy, tf[9], wx * tf[8]); }
#pragma unroll
        for (int q = 0; q < ZPL; ++q) {
            const double wzd = zv[q] - gz;
            const float wz = (float)wzd;
            const float d2 = fmaf(wz, wz, r2);
            const float d2c = fmaxf(d2, P.dmin2);
            const float ri = __builtin_amdgcn_rsqf(d2c);      // 1 / d'
            float t = amp * ri;
            bool act = true;
            if constexpr (KIND != STEER_UNIFORM) {
                const double cxd = fma(-wzd, ndy, cx0d), cyd = fma(wzd, ndx, cy0d);
                const double c2d = fma(cxd, cxd, fma(cyd, cyd, cz2d));
                const double d2d = fma(wzd, wzd, r2d);
                if constexpr (KIND == STEER_MAXANGLE) act = c2d <= P.lim2 * d2d;            // theta <= theta_max (theta = 0 at d = 0)
                else act = (c2d < P.lim2 * d2d) || d2d == 0.0;                              // theta < zero: a_e > 0
            }
            if constexpr (KIND == STEER_PIECEWISE) {
                const float cx = fmaf(-wz, nfy, cx0), cy = fmaf(wz, nfx, cy0);
                const float c2 = fmaf(cx, cx, fmaf(cy, cy, cz2));
                const float s2 = d2 > 0.f ? c2 * __builtin_amdgcn_rcpf(d2) : 0.f;
                const float th = asinf(__builtin_sqrtf(fminf(s2, 1.0f)));
                t *= fminf(fmaxf(fmaf(-P.pw_scale, th, P.pw_off), 0.f), 1.0f);
            }
            if constexpr (DIRECTIVITY) t *= piston_dir(fmaf(wz, tf[6], px), fmaf(wz, tf[10], py), ri, tf[7], tf[11]);
            if constexpr (ABSORB) t *= __builtin_amdgcn_exp2f(-P.absorb_l2 * (d2c * ri));      // exp(-alpha d')
            acc[q] += act ? t : 0.f;
            if constexpr (KIND != STEER_UNIFORM) cnt[q] += act ? 1 : 0;
        }
    }
    if constexpr (KIND == STEER_UNIFORM) {
#pragma unroll
        for (int q = 0; q < ZPL; ++q) { acc[q] *= P.value; cnt[q] = P.value > 0.f ? P.n_el : 0; }
    }
    const long long base = row * P.nz + k0;
    if (k0 + ZPL <= P.nz) {      // (dword-aligned 16-byte stores: rows of odd length are fine)
        if (OLX_IN(base, P.vox, 0) && OLX_IN(base + ZPL - 1, P.vox, 0)) *reinterpret_cast<floatx4u_t*>(pfocal + base) = floatx4u_t{acc[0], acc[1], acc[2], acc[3]};
        if (OLX_IN(base, P.vox, 1) && OLX_IN(base + ZPL - 1, P.vox, 1)) *reinterpret_cast<intx4u_t*>(nact + base) = intx4u_t{cnt[0], cnt[1], cnt[2], cnt[3]};
    } else {
#pragma unroll
        for (int q = 0; q < ZPL; ++q) {
            if (k0 + q < P.nz) {
                if (OLX_IN(base + q, P.vox, 2)) pfocal[base + q] = acc[q];
                if (OLX_IN(base + q, P.vox, 3)) nact[base + q] = cnt[q];
            }
        }
    }
}

OLX_BOUNDS_READER(steer)

}  // namespace olx

using namespace olx;

template <int KIND>
static void launch_steer_kind(olx_ctx* c, const SteerParams& P, bool dir, bool absorb, dim3 grid) {
    const dim3 blk(FIELD_THREADS);
    double* td = c->d_sm_tabd; float* tf = c->d_sm_tabf; float* pf = c->d_sm_p; int* na = c->d_sm_n;
    if (dir) {
        if (absorb) hipLaunchKernelGGL((steer_map_k<KIND, true, true>), grid, blk, 0, c->stream, td, tf, pf, na, P);
        else        hipLaunchKernelGGL((steer_map_k<KIND, true, false>), grid, blk, 0, c->stream, td, tf, pf, na, P);
    } else {
        if (absorb) hipLaunchKernelGGL((steer_map_k<KIND, false, true>), grid, blk, 0, c->stream, td, tf, pf, na, P);
        else        hipLaunchKernelGGL((steer_map_k<KIND, false, false>), grid, blk, 0, c->stream, td, tf, pf, na, P);
    }
}

void olx_launch_steer_table(olx_ctx* c, const double* apertures, double wscale, double inv_2lambda) {
    hipLaunchKernelGGL(steer_table_k, dim3((c->n_el + 255) / 256), dim3(256), 0, c->stream, c->d_pos, c->d_nrm, c->d_area, apertures, c->n_el, wscale,
                       inv_2lambda, (double*)c->d_sm_tabd, (float*)c->d_sm_tabf);
}

void olx_launch_steer_map(olx_ctx* c, const SteerParams& P0, int kind, bool dir) {
    SteerParams P = P0;
#ifdef OLX_DEBUG_BOUNDS   // self-test of the debug library: a wrong extent must be reported
    if (getenv("OLX_DEBUG_BOUNDS_SELFTEST")) P.vox -= 1;
#endif
    const long long lanes = (long long)P.nx * P.ny * ((P.nz + 3) / 4);
    const dim3 grid((unsigned)((lanes + FIELD_THREADS - 1) / FIELD_THREADS));
    const bool absorb = P.absorb_l2 > 0.f;
    if (kind == STEER_UNIFORM) launch_steer_kind<STEER_UNIFORM>(c, P, dir, absorb, grid);
    else if (kind == STEER_MAXANGLE) launch_steer_kind<STEER_MAXANGLE>(c, P, dir, absorb, grid);
    else launch_steer_kind<STEER_PIECEWISE>(c, P, dir, absorb, grid);
}
