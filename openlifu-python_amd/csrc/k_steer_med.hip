// kernel 4h (steer_map_med_k): the steering map through a heterogeneous medium, straight rays -- focal pressure when the array is steered to
// each voxel THROUGH the medium.  gfx950 (CDNA4, wave64) only.  Definition: DESIGN.md section 2 ("Steering map through a medium"), fp64 oracle
// tests/steering_medium_oracle.py.
//
// Per candidate voxel v = (i, j, kv) and element e, with w, d, d' = max(d, dmin), the folded angle, the base apodization b_e, S_e and the piston
// factor D_e exactly as kernel 4 forms them (k_steer.hip: same expressions, same fp64 decisions):
//     A_e = 0 if z_v == z_e, else l (a(v) / 2 + sum_{k in K} a_k(crossing_k)),  l = hz d' / |z_v - z_e|        E_e = the same sum over sig = c_ref / c - 1
//     K   = kfirst_e <= k < kv (voxel above the element) | kv < k <= klast_e (below): kernel 2h's host-decided plane bounds
//     h_e = exp(-A_e) [S_e / d' with spreading];  c_e = b_e | b_e min_active(h) / h_e (equalize) | b_e h_e / max_active(h) (matched)
//     P   = (P0 / lambda) sum_e c_e S_e D_e exp(-A_e) / d'                                      (StraightRay delays: every term in phase)
//     P   = (P0 / lambda) | sum_e c_e S_e D_e exp(-A_e) / d' exp(j 2 pi E_e / lambda) |         (Direct delays: PHASE)
// ONE walk of the rays per (lane, element) serves every mode: min / max of h over the active elements of a voxel do not depend on e, so
//     equalize:  P = hmin sum_e b_e S_e D_e / d' (exp(-A_e) / h_e),     matched:  P = sum_e b_e S_e D_e / d' exp(-A_e) h_e / hmax
// and the sums, hmin and hmax accumulate in the one pass over the elements.
//
// The medium is kernel 2h's PRE-GATHERED bilinear stencil (k_hetero.hip): texel (p, i, j) = { sig, a' } x {(i,j), (i,j+1), (i+1,j), (i+1,j+1)},
// edge-clamped, 32 bytes, over the non-trivial planes only; a' = a lambda [Np per wavelength] and l in wavelengths, so that l sum sig is the
// phase in revolutions.  Work map as kernel 2h: a wave = an 8 x 8 (x, y) tile of voxels x 4 consecutive z per lane, the four waves of a block
// = four consecutive z chunks of the tile; the plane loops are wave-uniform.  Precision: w from fp64 (integer index, fp64 element position)
// rounded once; decisions in fp64; plane bounds are the host's integers; stencil values fp64 rounded once; everything else fp32.  The
// PHASE = false instantiations carry no sig arithmetic and no sin / cos.
//
// Bounds sites of the debug library: 0 / 1 the 16-byte stores of P / n_active, 2 / 3 their dword tails, 4 stencil texels, 5 the plane list,
// 6 the plane map.
#include "k_types.hip.h"
#include "olx_ctx.h"
#include "olx_launch.h"

namespace olx {

typedef int smm_i4u_t __attribute__((ext_vector_type(4), aligned(4)));
typedef float smm_f4_t __attribute__((ext_vector_type(4), aligned(16)));

enum { SMM_UNIFORM = 0, SMM_MAXANGLE = 1, SMM_PIECEWISE = 2 };
enum { SMM_NONE = 0, SMM_EQUALIZE = 1, SMM_MATCHED = 2 };

// one bilinear, border-extended sample of a stencil plane (every cell carries its own 2 x 2 stencil: u = n - 1 is a valid cell with weight 0)
template <bool SIG>
__device__ __forceinline__ void smm_sample(const char* __restrict__ plane, long long plane_bytes, float tt, float dxu, float dyv, float eu, float ev,
                                           float umax, float vmax, int nyg, float& ss, float& as) {
    const float u = __builtin_amdgcn_fmed3f(fmaf(tt, dxu, eu), 0.f, umax);
    const float v = __builtin_amdgcn_fmed3f(fmaf(tt, dyv, ev), 0.f, vmax);
    const unsigned i0 = (unsigned)(int)u, j0 = (unsigned)(int)v;
    const float fu = __builtin_amdgcn_fractf(u), fv = __builtin_amdgcn_fractf(v);
    const unsigned off = (__umul24(i0, (unsigned)nyg) + j0) << 5;            // 32 bytes per cell
    if (!OLX_IN((long long)off + 31, plane_bytes, 4)) return;
    const smm_f4_t lo = *reinterpret_cast<const smm_f4_t*>(plane + off), hi = *reinterpret_cast<const smm_f4_t*>(plane + off + 16);
    // {s00,a00,s01,a01}, {s10,a10,s11,a11}
    const float a0 = fmaf(fv, lo.w - lo.y, lo.y), a1 = fmaf(fv, hi.w - hi.y, hi.y);
    as += fmaf(fu, a1 - a0, a0);
    if constexpr (SIG) {
        const float s0 = fmaf(fv, lo.z - lo.x, lo.x), s1 = fmaf(fv, hi.z - hi.x, hi.x);
        ss += fmaf(fu, s1 - s0, s0);
    }
}

template <int KIND, int COMP, bool PHASE, bool DIRECTIVITY>
__global__ __launch_bounds__(FIELD_THREADS) void steer_map_med_k(const double* __restrict__ tabd, const float* __restrict__ tabf, const float* __restrict__ tabm,
                                                                 const float4* __restrict__ med, const int* __restrict__ plane_k,
                                                                 const int* __restrict__ plane_of_k, float* __restrict__ pfocal, int* __restrict__ nact,
                                                                 const SteerMedParams M) {
    constexpr int ZPL = 4;
    const SteerParams& P = M.S;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tiles_y = (P.ny + 7) >> 3, zblocks = (P.nz + 4 * ZPL - 1) / (4 * ZPL);
    const int zb = blockIdx.x % zblocks;
    const int tile = blockIdx.x / zblocks;
    const int ti = tile / tiles_y, tj = tile - ti * tiles_y;
    const int i = ti * 8 + (lane >> 3), j = tj * 8 + (lane & 7);
    const int k0 = (zb * 4 + wave) * ZPL;                                   // wave-uniform
    if (k0 >= P.nz) return;                                                 // (the whole wave)
    const bool live = i < P.nx && j < P.ny;
    const int ic = min(i, P.nx - 1), jc = min(j, P.ny - 1);
    const double xv = P.ox + ic * P.hx, yv = P.oy + jc * P.hy;
    const size_t plane_sz = (size_t)P.nx * P.ny * 2;                        // float4 per plane
    const long long plane_bytes = (long long)plane_sz * 16;
    const float umax = (float)(P.nx - 1), vmax = (float)(P.ny - 1);
    double zv[ZPL];
    float re[ZPL], im[ZPL], hm[ZPL], sv[ZPL], av[ZPL];
    int cnt[ZPL];
#pragma unroll
    for (int q = 0; q < ZPL; ++q) {
        const int kq = min(k0 + q, P.nz - 1);
        zv[q] = P.oz + (k0 + q) * P.hz;
        re[q] = 0.f; im[q] = 0.f; cnt[q] = 0;
        hm[q] = COMP == SMM_EQUALIZE ? INFINITY : -INFINITY;
        const int pq = OLX_IN(kq, P.nz, 6) ? plane_of_k[kq] : -1;           // the voxel's own half layer
        float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
        if (pq >= 0 && OLX_IN(pq, M.n_planes, 5)) m = med[((size_t)pq * P.nx + ic) * P.ny * 2 + (size_t)jc * 2];
        sv[q] = 0.5f * m.x; av[q] = 0.5f * m.y;
    }
    for (int e = 0; e < P.n_el; ++e) {
        const double* td = tabd + (size_t)e * STEER_TD;
        const float* tf = tabf + (size_t)e * STEER_TF;
        const float* tm = tabm + (size_t)e * STEER_TM;
        const int kfirst = __float_as_int(tm[0]), klast = __float_as_int(tm[1]);
        const double wxd = xv - td[0], wyd = yv - td[1], gz = td[2];
        const float wx = (float)wxd, wy = (float)wyd;
        const float r2 = fmaf(wy, wy, wx * wx);
        const float amp = tf[3];
        // the crossing of plane k in grid index space: (eu, ev) + t (dxu, dyv), t = (z_k - z_e) / (z_v - z_e)
        const float eu = (float)((td[0] - P.ox) * M.inv_hx), ev = (float)((td[1] - P.oy) * M.inv_hy);
        const float dxu = (float)(wxd * M.inv_hx), dyv = (float)(wyd * M.inv_hy);
        // the parts of w x n, |w|^2 and w . ex, w . ey that do not depend on z (kernel 4's)
        double ndx = 0, ndy = 0, cx0d = 0, cy0d = 0, cz2d = 0, r2d = 0;
        if constexpr (KIND != SMM_UNIFORM) {
            ndx = td[4]; ndy = td[5];
            const double ndz = td[6], czd = wxd * ndy - wyd * ndx;
            cx0d = wyd * ndz; cy0d = -wxd * ndz; cz2d = czd * czd;
            r2d = fma(wyd, wyd, wxd * wxd);
        }
        float nfx = 0, nfy = 0, cx0 = 0, cy0 = 0, cz2 = 0;
        if constexpr (KIND == SMM_PIECEWISE) {
            nfx = tf[0]; nfy = tf[1];
            const float nfz = tf[2], cz = fmaf(wx, nfy, -wy * nfx);
            cx0 = wy * nfz; cy0 = -wx * nfz; cz2 = cz * cz;
        }
        float px = 0, py = 0;
        if constexpr (DIRECTIVITY) { px = fmaf(wy, tf[5], wx * tf[4]); py = fmaf(wy, tf[9], wx * tf[8]); }
        double wzd[ZPL];
        float wz[ZPL], idz[ZPL], ss[ZPL], as[ZPL];
#pragma unroll
        for (int q = 0; q < ZPL; ++q) {
            wzd[q] = zv[q] - gz;
            wz[q] = (float)wzd[q];
            idz[q] = wz[q] != 0.f ? __builtin_amdgcn_rcpf(wz[q]) : 0.f;
            ss[q] = sv[q]; as[q] = av[q];
        }
        // planes between element and voxel: k in [kfirst, kv) (voxel above) or (kv, klast] (voxel below); k0, kfirst, klast are wave-uniform,
        // so every trip bound and branch below is too
        for (int p = 0; p < M.n_planes; ++p) {
            const int k = plane_k[p];
            const bool any_above = k >= kfirst && k < k0 + ZPL - 1, any_below = k <= klast && k > k0;
            if (!any_above && !any_below) continue;
            const float zk = (float)((P.oz + k * P.hz) - gz);
            const char* plane = reinterpret_cast<const char*>(med + (size_t)p * plane_sz);
#pragma unroll
            for (int q = 0; q < ZPL; ++q) {
                const int kv = k0 + q;
                const bool between = (k >= kfirst && k < kv) || (k <= klast && k > kv);
                if (!between) continue;
                smm_sample<PHASE>(plane, plane_bytes, zk * idz[q], dxu, dyv, eu, ev, umax, vmax, P.ny, ss[q], as[q]);
            }
        }
#pragma unroll
        for (int q = 0; q < ZPL; ++q) {
            const float d2 = fmaf(wz[q], wz[q], r2);
            const float d2c = fmaxf(d2, P.dmin2);
            const float ri = __builtin_amdgcn_rsqf(d2c);      // 1 / d'
            const float dc = d2c * ri;                        // d'
            float t = amp * ri;
            bool act = true;
            if constexpr (KIND != SMM_UNIFORM) {
                const double cxd = fma(-wzd[q], ndy, cx0d), cyd = fma(wzd[q], ndx, cy0d);
                const double c2d = fma(cxd, cxd, fma(cyd, cyd, cz2d));
                const double d2d = fma(wzd[q], wzd[q], r2d);
                if constexpr (KIND == SMM_MAXANGLE) act = c2d <= P.lim2 * d2d;            // theta <= theta_max (theta = 0 at d = 0)
                else act = (c2d < P.lim2 * d2d) || d2d == 0.0;                            // theta < zero: b_e > 0
            }
            if constexpr (KIND == SMM_PIECEWISE) {
                const float cx = fmaf(-wz[q], nfy, cx0), cy = fmaf(wz[q], nfx, cy0);
                const float c2 = fmaf(cx, cx, fmaf(cy, cy, cz2));
                const float s2 = d2 > 0.f ? c2 * __builtin_amdgcn_rcpf(d2) : 0.f;
                const float th = asinf(__builtin_sqrtf(fminf(s2, 1.0f)));
                t *= fminf(fmaxf(fmaf(-P.pw_scale, th, P.pw_off), 0.f), 1.0f);
            }
            if constexpr (DIRECTIVITY) t *= piston_dir(fmaf(wz[q], tf[6], px), fmaf(wz[q], tf[10], py), ri, tf[7], tf[11]);
            const float lw = wz[q] != 0.f ? M.hz_w * dc * fabsf(idz[q]) : 0.f;            // l [wavelengths]; z_v == z_e: A = E = 0
            const float ea = __expf(-lw * as[q]);
            float contrib;
            if constexpr (COMP == SMM_NONE) {
                contrib = t * ea;
            } else {
                const float h = M.spreading ? ea * (tm[2] * ri) : ea;
                if constexpr (COMP == SMM_EQUALIZE) {
                    contrib = M.spreading ? t * (dc * tm[3]) : t;                          // t exp(-A) / h
                    if (act) hm[q] = fminf(hm[q], h);
                } else {
                    contrib = t * ea * h;
                    if (act) hm[q] = fmaxf(hm[q], h);
                }
            }
            contrib = act ? contrib : 0.f;
            if constexpr (PHASE) {
                const float ph = __builtin_amdgcn_fractf(lw * ss[q]);                      // E / lambda [revolutions]
                re[q] = fmaf(contrib, __builtin_amdgcn_cosf(ph), re[q]);
                im[q] = fmaf(contrib, __builtin_amdgcn_sinf(ph), im[q]);
            } else {
                re[q] += contrib;
            }
            if constexpr (KIND != SMM_UNIFORM) cnt[q] += act ? 1 : 0;
        }
    }
    float out[ZPL];
#pragma unroll
    for (int q = 0; q < ZPL; ++q) {
        if constexpr (KIND == SMM_UNIFORM) cnt[q] = P.value > 0.f ? P.n_el : 0;
        float v = PHASE ? __builtin_sqrtf(fmaf(re[q], re[q], im[q] * im[q])) : re[q];
        if constexpr (KIND == SMM_UNIFORM) v *= PHASE ? M.abs_value : P.value;
        if constexpr (COMP == SMM_EQUALIZE) v = cnt[q] > 0 ? v * hm[q] : 0.f;
        if constexpr (COMP == SMM_MATCHED) v = cnt[q] > 0 ? v / hm[q] : 0.f;
        out[q] = v;
    }
    if (!live) return;
    const long long base = ((long long)i * P.ny + j) * P.nz + k0;
    if (k0 + ZPL <= P.nz) {      // (dword-aligned 16-byte stores: rows of odd length are fine)
        if (OLX_IN(base, P.vox, 0) && OLX_IN(base + ZPL - 1, P.vox, 0)) *reinterpret_cast<floatx4u_t*>(pfocal + base) = floatx4u_t{out[0], out[1], out[2], out[3]};
        if (OLX_IN(base, P.vox, 1) && OLX_IN(base + ZPL - 1, P.vox, 1)) *reinterpret_cast<smm_i4u_t*>(nact + base) = smm_i4u_t{cnt[0], cnt[1], cnt[2], cnt[3]};
    } else {
#pragma unroll
        for (int q = 0; q < ZPL; ++q) {
            if (k0 + q < P.nz) {
                if (OLX_IN(base + q, P.vox, 2)) pfocal[base + q] = out[q];
                if (OLX_IN(base + q, P.vox, 3)) nact[base + q] = cnt[q];
            }
        }
    }
}

OLX_BOUNDS_READER(steermed)

}  // namespace olx

using namespace olx;

template <int KIND, int COMP, bool PHASE>
static void launch_smm_dir(olx_ctx* c, const SteerMedParams& M, bool dir, dim3 grid) {
    const dim3 blk(FIELD_THREADS);
    if (dir) hipLaunchKernelGGL((steer_map_med_k<KIND, COMP, PHASE, true>), grid, blk, 0, c->stream, c->d_sm_tabd, c->d_sm_tabf, c->d_smm_tabm, c->d_smm_med,
                                c->d_smm_plane_k, c->d_smm_plane_of_k, c->d_smm_p, c->d_smm_n, M);
    else     hipLaunchKernelGGL((steer_map_med_k<KIND, COMP, PHASE, false>), grid, blk, 0, c->stream, c->d_sm_tabd, c->d_sm_tabf, c->d_smm_tabm, c->d_smm_med,
                                c->d_smm_plane_k, c->d_smm_plane_of_k, c->d_smm_p, c->d_smm_n, M);
}

template <int KIND, int COMP>
static void launch_smm_phase(olx_ctx* c, const SteerMedParams& M, bool phase, bool dir, dim3 grid) {
    if (phase) launch_smm_dir<KIND, COMP, true>(c, M, dir, grid);
    else       launch_smm_dir<KIND, COMP, false>(c, M, dir, grid);
}

template <int KIND>
static void launch_smm_comp(olx_ctx* c, const SteerMedParams& M, int comp, bool phase, bool dir, dim3 grid) {
    if (comp == SMM_NONE) launch_smm_phase<KIND, SMM_NONE>(c, M, phase, dir, grid);
    else if (comp == SMM_EQUALIZE) launch_smm_phase<KIND, SMM_EQUALIZE>(c, M, phase, dir, grid);
    else launch_smm_phase<KIND, SMM_MATCHED>(c, M, phase, dir, grid);
}

// comp: 0 none, 1 equalize, 2 matched
void olx_launch_steer_map_medium(olx_ctx* c, const SteerMedParams& M0, int kind, int comp, bool phase, bool dir) {
    SteerMedParams M = M0;
#ifdef OLX_DEBUG_BOUNDS   // self-test of the debug library: a wrong extent must be reported
    if (getenv("OLX_DEBUG_BOUNDS_SELFTEST")) M.S.vox -= 1;
#endif
    const long long nblk = (long long)((M.S.nx + 7) / 8) * ((M.S.ny + 7) / 8) * ((M.S.nz + 15) / 16);   // 8 x 8 tile x 16 z
    const dim3 grid((unsigned)nblk);
    if (kind == SMM_UNIFORM) launch_smm_comp<SMM_UNIFORM>(c, M, comp, phase, dir, grid);
    else if (kind == SMM_MAXANGLE) launch_smm_comp<SMM_MAXANGLE>(c, M, comp, phase, dir, grid);
    else launch_smm_comp<SMM_PIECEWISE>(c, M, comp, phase, dir, grid);
}
