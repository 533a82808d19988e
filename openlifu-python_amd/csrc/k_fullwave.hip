// kernel 5 (fullwave_pack_k, fullwave_inject_k, fullwave_vel_k, fullwave_pres_k, fullwave_trace_k, fullwave_receive_k; element apertures:
// fullwave_aperture_k, fullwave_drive_k, fullwave_inject_elem_k; response drive: fullwave_drive_fir_k): full-wave FDTD field model --
// linear acoustics, first order in (p, v) on a staggered grid, second order in time, fourth order in space.
// gfx950 (CDNA4, wave64) only.  Definition: DESIGN.md section 2 ("full-wave model") and section 5.14, fp64 oracle tests/fullwave_oracle.py.
//
// p lives at voxel centres, v_a on the + face along axis a, stored at the voxel's index (C order, z fastest); any field read outside
// the grid is 0.  State (p^n, v^(n - 1/2)), fp32.  Step n, one launch each, in place:
//   inject    p[vox_s] += amp_s env(u) sin(2 pi f0 u), u = (n - 1/2) dt - tau_s, for the entries with 0 <= u < T (decided, and the phase
//             reduced, in fp64); ONE thread per distinct source voxel walks its entries in table order (CSR): no atomics, no race
//   velocity  v_a <- D (v_a - b_a d+_a p),  d+ p[i] = 9/8 (p[i+1] - p[i]) - 1/24 (p[i+2] - p[i-1]),  b_a = dt / (rho_face h_a)
//             (each lane reads p around it and reads / writes only its own v: in place)
//   pressure  p~ <- g (p - kp sum_a d-_a v_a / h_a),  d- v[i] = 9/8 (v[i] - v[i-1]) - 1/24 (v[i+1] - v[i-2]),  kp = dt rho c^2, g = D ga,
//             ga = exp(-2 alpha c dt); then p_max = max(p_max, p~), p_min = max(p_min, -p~) and, opt-in, sum += p~^2 (one fmaf)
//             (each lane reads v around it and reads / writes only its own p: in place)
//   trace     opt-in: p~ at the trace voxels into row n
//   lock-in   opt-in, for the steps n of a window only: theta_n = 2 pi frac(f0 (n + 1) dt) formed in fp64 on the host;
//             volume: C += p~ cosf_n, S += p~ sinf_n (one fmaf each, cos / sin theta_n rounded once to float and passed as kernel arguments),
//             the third template flag of the pressure launch; receivers: s_r = sum_q w_q p~(vox_q) in table order, C_r += s_r cos theta_n,
//             S_r += s_r sin theta_n in fp64, ONE thread per receiver walking its CSR row (the form of inject: no atomics)
//   apertures opt-in: fullwave_aperture_k spreads each element's rectangle over the voxels (weights W_e(m), fp64, once per
//             geometry); the sources then stand in element-factored form -- entries (voxel, element, amp_{e,m}) and a drive table s_e(n) filled
//             by ONE launch of fullwave_drive_k -- and fullwave_inject_elem_k takes the place of inject: p[vox] += (float)(amp_{e,m} s_e(n))
//   drives    opt-in (DESIGN.md section 2 "full-wave model: drives", section 5.20): the drive table of the element-factored form is filled with the bare
//             burst (fullwave_drive_k), with the burst through per-class drive taps (fullwave_drive_k over the steps -(M_max - 1) .. n_steps - 1, then
//             fullwave_drive_fir_k), or with sampled waveforms as uploaded; the step loop reads the table and is the same for all three
// D = d_x[i] d_y[j] d_z[k] from three 1-D tables (1 in the interior, the absorbing layers' decay per step outside it).
// Split layers (opt-in, olx_fullwave_layers; DESIGN.md section 2 "full-wave model: split layers", section 5.19): two 1-D tables per axis take the place
// of d -- s_a (face depth) for the velocity launch fullwave_vel_k<UNI, SPLIT>, v_a <- s_a (s_a v_a - b_a d+_a p), and r_a (centre depth) for the
// pressure launch, a kernel of its own (fullwave_pres_split_k; fullwave_pres_k is untouched), which in a layer voxel advances three components p_a <- ga (r_a (r_a p_a - (kp d-_a v_a) / h_a)) and stores p~ = (p_x + p_y) + p_z;
// an interior voxel takes the update above with D = 1 and touches no component.
// A heterogeneous medium streams five coefficient volumes formed once by fullwave_pack_k (b_x, b_y, b_z for the velocity launch, kp, ga
// for the pressure launch); the uniform instantiation (UNI) streams none of them.
#include "k_types.hip.h"
#include "olx_ctx.h"
#include "olx_launch.h"

namespace olx {

constexpr int FW_BLOCK = 256;
constexpr float FW_C1 = 9.0f / 8.0f, FW_C2 = 1.0f / 24.0f;

// (i, j, k) of linear voxel v (vox < 2^31: two 32-bit divisions)
__device__ __forceinline__ void fw_ijk(unsigned v, const FullwaveParams& P, int& i, int& j, int& k) {
    const unsigned row = v / (unsigned)P.nz;
    k = (int)(v - row * (unsigned)P.nz);
    i = (int)(row / (unsigned)P.ny);
    j = (int)(row - (unsigned)i * (unsigned)P.ny);
}

// a[u], u inside the volume by the caller's index test (checked against the extent in the debug library); 0 when the test fails
__device__ __forceinline__ float fw_ld(const float* __restrict__ a, bool inside, long long u, long long vox, int site) {
    return (inside && OLX_IN(u, vox, site)) ? a[u] : 0.f;
}

__device__ __forceinline__ float fw_layer(const float* __restrict__ dtab, const FullwaveParams& P, int i, int j, int k) {
    const int n = P.nx + P.ny + P.nz;
    float d = 1.f;
    if (OLX_IN(i, n, 20) && OLX_IN(P.nx + j, n, 20) && OLX_IN(P.nx + P.ny + k, n, 20)) d = (dtab[i] * dtab[P.nx + j]) * dtab[P.nx + P.ny + k];
    return d;
}

// coefficient volumes of a heterogeneous medium (NULL volume = the scalar of FullwaveParams): b_a = dt / (rho_face h_a) with rho_face the
// mean of the two voxels' rho (the voxel's own on the high boundary), kp = dt rho c^2, ga = exp(-2 alpha c dt)
__global__ __launch_bounds__(FW_BLOCK) void fullwave_pack_k(const float* __restrict__ cs, const float* __restrict__ rho, const float* __restrict__ alpha,
                                                            const FullwaveParams P, float* __restrict__ bx, float* __restrict__ by,
                                                            float* __restrict__ bz, float* __restrict__ kp, float* __restrict__ ga) {
    const long long v = (long long)blockIdx.x * FW_BLOCK + threadIdx.x;
    if (v >= P.vox) return;
    int i, j, k;
    fw_ijk((unsigned)v, P, i, j, k);
    const long long pl = (long long)P.ny * P.nz;
    auto rv = [&](bool inside, long long u, float own) { return rho ? (inside && OLX_IN(u, P.vox, 0) ? rho[u] : own) : P.rho0; };
    if (!OLX_IN(v, P.vox, 1)) return;
    const float r = rho ? rho[v] : P.rho0, c = cs ? cs[v] : P.c0, a = alpha ? alpha[v] : P.alpha0;
    bx[v] = P.dthx / (0.5f * (r + rv(i + 1 < P.nx, v + pl, r)));
    by[v] = P.dthy / (0.5f * (r + rv(j + 1 < P.ny, v + P.nz, r)));
    bz[v] = P.dthz / (0.5f * (r + rv(k + 1 < P.nz, v + 1, r)));
    kp[v] = P.dt * r * c * c;
    ga[v] = expf(-2.0f * a * c * P.dt);
}

// the sources of step n: row r of the CSR table is one voxel, its entries add in table order
__global__ void fullwave_inject_k(float* __restrict__ p, const long long* __restrict__ svox, const int* __restrict__ srow, const double* __restrict__ samp,
                                  const double* __restrict__ stau, const FullwaveSource S, int n_entries, long long vox, int step) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= S.n_vox || !OLX_IN(r + 1, S.n_vox + 1, 2)) return;
    const long long at = svox[r];
    if (!OLX_IN(at, vox, 3)) return;
    float acc = p[at];
    bool any = false;
    for (int e = srow[r]; e < srow[r + 1]; ++e) {
        if (!OLX_IN(e, n_entries, 4)) break;
        const double u = ((double)step - 0.5) * S.dt - stau[e];
        if (!(u >= 0.0 && u < S.T)) continue;
        double ph = S.freq * u;
        ph -= floor(ph);
        double env = 1.0;
        if (S.Tr > 0.0) {
            if (u < S.Tr) env *= 0.5 * (1.0 - cos(M_PI * u / S.Tr));
            if (S.T - u < S.Tr) env *= 0.5 * (1.0 - cos(M_PI * (S.T - u) / S.Tr));
        }
        acc += (float)(samp[e] * env * sin(2.0 * M_PI * ph));
        any = true;
    }
    if (any) p[at] = acc;
}

// element-factored sources: the drive s_e(n) of every (step, element), one lane each, formed as fullwave_inject_k forms
// it and exactly 0.0 outside the burst; the step loop then holds no trigonometry.  Lane g holds row g / n_el of the table, which is step
// n = n0 + row (n0 = 0 for the drive table itself, -(M_max - 1) for the extended bare table of the response drive: a negative n goes through
// the same expression), and writes drive[row ns + e es]: (ns, es) = (n_el, 1) is the step-major drive table, (1, rows) the element-major
// extended table that fullwave_drive_fir_k reads along n.
__global__ __launch_bounds__(FW_BLOCK) void fullwave_drive_k(const double* __restrict__ A, const double* __restrict__ tau, const FullwaveSource S, int n_el,
                                                             long long total, long long n0, long long ns, long long es, double* __restrict__ drive) {
    const long long g = (long long)blockIdx.x * FW_BLOCK + threadIdx.x;
    if (g >= total || !OLX_IN(g, total, 21)) return;
    const long long row = g / n_el;
    const int e = (int)(g - row * n_el);
    const long long n = n0 + row, at = row * ns + e * es;
    if (!OLX_IN(e, n_el, 22) || !OLX_IN(at, total, 32)) return;
    const double u = ((double)n - 0.5) * S.dt - tau[e];
    double s = 0.0;
    if (u >= 0.0 && u < S.T) {
        double ph = S.freq * u;
        ph -= floor(ph);
        double env = 1.0;
        if (S.Tr > 0.0) {
            if (u < S.Tr) env *= 0.5 * (1.0 - cos(M_PI * u / S.Tr));
            if (S.T - u < S.Tr) env *= 0.5 * (1.0 - cos(M_PI * (S.T - u) / S.Tr));
        }
        s = A[e] * env * sin(2.0 * M_PI * ph);
    }
    drive[at] = s;
}

// the response drive (DESIGN.md section 2 "full-wave model: drives"): s_e(n) = sum_{m < M_c} g_c[m] s0_e(n - m), c the class of element e, in
// fp64 with m ascending from 0.0, every product and sum rounded on its own -- taps [1.0] give s0_e(n) bit for bit.  One block is one element and
// FW_BLOCK consecutive steps, so the whole block shares a class: its taps (at most FW_FIR_TAPS) are staged in LDS once, and a wave reads 64
// consecutive doubles of the element-major extended table ext[n_el][rows] (rows = n_steps + lead, row lead + n = step n) per tap.
constexpr int FW_FIR_TAPS = 256;     // OLX_PULSE_RESPONSE_MAX_TAPS
__global__ __launch_bounds__(FW_BLOCK) void fullwave_drive_fir_k(const double* __restrict__ ext, const int* __restrict__ cls, const int* __restrict__ row,
                                                                 const double* __restrict__ taps, int n_el, int n_classes, int n_taps, int n_steps, int lead,
                                                                 double* __restrict__ drive) {
#pragma clang fp contract(off)
    __shared__ double g_s[FW_FIR_TAPS];
    const int e = (int)(blockIdx.x % (unsigned)n_el);
    const long long n = (long long)(blockIdx.x / (unsigned)n_el) * FW_BLOCK + threadIdx.x;
    // (every return before the barrier is taken by the whole block: e, c and M are the block's)
    if (!OLX_IN(e, n_el, 33)) return;
    const int c = cls[e];
    if (!OLX_IN(c, n_classes, 34)) return;
    const int r0 = row[c], M = row[c + 1] - r0;
    if (!OLX_IN(M - 1, FW_FIR_TAPS, 35) || !OLX_IN(M - 1, lead + 1, 35) || !OLX_IN(r0 + M - 1, n_taps, 36) || !OLX_IN(r0, n_taps, 36)) return;
    for (int t = threadIdx.x; t < M; t += FW_BLOCK) g_s[t] = taps[r0 + t];
    __syncthreads();
    if (n >= n_steps) return;
    const long long rows = (long long)n_steps + lead, base = (long long)e * rows + lead + n;
    double acc = 0.0;
    for (int m = 0; m < M; ++m) {
        if (!OLX_IN(base - m, (long long)n_el * rows, 37)) break;
        acc = acc + g_s[m] * ext[base - m];
    }
    const long long at = n * n_el + e;
    if (OLX_IN(at, (long long)n_steps * n_el, 38)) drive[at] = acc;
}

// the sources of step n in element-factored form: row r of the CSR table is one voxel, its entries (amp_{e,m}, e) add in table order
__global__ void fullwave_inject_elem_k(float* __restrict__ p, const long long* __restrict__ svox, const int* __restrict__ srow, const double* __restrict__ samp,
                                       const int* __restrict__ sel, const double* __restrict__ drive, int n_vox, int n_entries, int n_el, long long n_drive,
                                       long long vox, int step) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_vox || !OLX_IN(r + 1, n_vox + 1, 23)) return;
    const long long at = svox[r];
    if (!OLX_IN(at, vox, 24)) return;
    float acc = p[at];
    bool any = false;
    for (int q = srow[r]; q < srow[r + 1]; ++q) {
        if (!OLX_IN(q, n_entries, 25)) break;
        const int e = sel[q];
        const long long d = (long long)step * n_el + e;
        if (!OLX_IN(e, n_el, 26) || !OLX_IN(d, n_drive, 27)) continue;
        const double s = drive[d];
        if (s == 0.0) continue;
        acc += (float)(samp[q] * s);
        any = true;
    }
    if (any) p[at] = acc;
}

// aperture weights in gather form: one lane per (element, voxel of the element's index box) walks the element's quadrature points in the
// order of the definition (a outer, b inner) and writes W_e(m) in fp64.  Every operation is rounded on its own (no contraction), so the
// coordinates are the bits that the host's refusals and the fp64 oracle see.
__global__ __launch_bounds__(FW_BLOCK) void fullwave_aperture_k(const FullwaveAperture* __restrict__ ap, int n_el, double ox, double oy, double oz, double hx,
                                                                double hy, double hz, double* __restrict__ W, long long total) {
#pragma clang fp contract(off)
    const int e = blockIdx.x;
    if (!OLX_IN(e, n_el, 28)) return;
    const FullwaveAperture E = ap[e];
    const long long t = (long long)blockIdx.y * FW_BLOCK + threadIdx.x;
    if (t >= (long long)E.dim[0] * E.dim[1] * E.dim[2]) return;
    const long long row = t / E.dim[2];
    const double mk = (double)(E.lo[2] + (int)(t - row * E.dim[2]));
    const double mj = (double)(E.lo[1] + (int)(row % E.dim[1]));
    const double mi = (double)(E.lo[0] + (int)(row / E.dim[1]));
    double acc = 0.0;
    for (int a = 0; a < E.nw; ++a) {
        const double sa = fw_aperture_s(a, E.nw);
        for (int b = 0; b < E.nl; ++b) {
            const double sb = fw_aperture_s(b, E.nl);
            const double dx = 1.0 - fabs(fw_aperture_q(E, sa, sb, 0, ox, hx) - mi);
            if (!(dx > 0.0)) continue;
            const double dy = 1.0 - fabs(fw_aperture_q(E, sa, sb, 1, oy, hy) - mj);
            if (!(dy > 0.0)) continue;
            const double dz = 1.0 - fabs(fw_aperture_q(E, sa, sb, 2, oz, hz) - mk);
            if (!(dz > 0.0)) continue;
            acc += (dx * dy) * dz;
        }
    }
    if (OLX_IN(E.off + t, total, 29)) W[E.off + t] = acc / (double)(E.nw * E.nl);
}

template <bool UNI, bool SPLIT = false>
__global__ __launch_bounds__(FW_BLOCK) void fullwave_vel_k(const float* __restrict__ p, float* __restrict__ vx, float* __restrict__ vy, float* __restrict__ vz,
                                                           const float* __restrict__ bx, const float* __restrict__ by, const float* __restrict__ bz,
                                                           const float* __restrict__ dtab, const FullwaveParams P) {
    const long long v = (long long)blockIdx.x * FW_BLOCK + threadIdx.x;
    if (v >= P.vox || !OLX_IN(v, P.vox, 5)) return;
    int i, j, k;
    fw_ijk((unsigned)v, P, i, j, k);
    const long long pl = (long long)P.ny * P.nz, nz = P.nz;
    float D = 1.f, sx = 1.f, sy = 1.f, sz = 1.f;
    if constexpr (SPLIT) {      // dtab is s_x | s_y | s_z: each component is damped by its own axis only
        const int n = P.nx + P.ny + P.nz;
        if (OLX_IN(i, n, 30) && OLX_IN(P.nx + j, n, 30) && OLX_IN(P.nx + P.ny + k, n, 30)) { sx = dtab[i]; sy = dtab[P.nx + j]; sz = dtab[P.nx + P.ny + k]; }
    } else {
        D = fw_layer(dtab, P, i, j, k);
    }
    const float pc = p[v];
    const float dpx = FW_C1 * (fw_ld(p, i + 1 < P.nx, v + pl, P.vox, 6) - pc) - FW_C2 * (fw_ld(p, i + 2 < P.nx, v + 2 * pl, P.vox, 6) - fw_ld(p, i > 0, v - pl, P.vox, 6));
    const float dpy = FW_C1 * (fw_ld(p, j + 1 < P.ny, v + nz, P.vox, 7) - pc) - FW_C2 * (fw_ld(p, j + 2 < P.ny, v + 2 * nz, P.vox, 7) - fw_ld(p, j > 0, v - nz, P.vox, 7));
    const float dpz = FW_C1 * (fw_ld(p, k + 1 < P.nz, v + 1, P.vox, 8) - pc) - FW_C2 * (fw_ld(p, k + 2 < P.nz, v + 2, P.vox, 8) - fw_ld(p, k > 0, v - 1, P.vox, 8));
    const float cbx = UNI ? P.bx0 : bx[v], cby = UNI ? P.by0 : by[v], cbz = UNI ? P.bz0 : bz[v];
    if constexpr (SPLIT) {
        // the fused multiply-add is spelled out: s_a v_a is rounded first and b_a d+ p enters unrounded, so that s_a = 1 gives the bits of the
        // update below (left to the compiler, s v - b dp may contract around the other product)
        vx[v] = sx * fmaf(-cbx, dpx, sx * vx[v]);
        vy[v] = sy * fmaf(-cby, dpy, sy * vy[v]);
        vz[v] = sz * fmaf(-cbz, dpz, sz * vz[v]);
    } else {
        vx[v] = D * (vx[v] - cbx * dpx);
        vy[v] = D * (vy[v] - cby * dpy);
        vz[v] = D * (vz[v] - cbz * dpz);
    }
}

// the lock-in arguments of the pressure launch; empty, and last, without LOCK: those instantiations keep their argument layout
template <bool LOCK> struct FwLock { float *c, *s; float cosf_n, sinf_n; };
template <> struct FwLock<false> {};

template <bool UNI, bool PII, bool LOCK>
__global__ __launch_bounds__(FW_BLOCK) void fullwave_pres_k(float* __restrict__ p, const float* __restrict__ vx, const float* __restrict__ vy,
                                                            const float* __restrict__ vz, const float* __restrict__ kp, const float* __restrict__ ga,
                                                            const float* __restrict__ dtab, float* __restrict__ pmax, float* __restrict__ pmin,
                                                            float* __restrict__ psq, const FullwaveParams P, const FwLock<LOCK> L) {
    const long long v = (long long)blockIdx.x * FW_BLOCK + threadIdx.x;
    if (v >= P.vox || !OLX_IN(v, P.vox, 9)) return;
    int i, j, k;
    fw_ijk((unsigned)v, P, i, j, k);
    const long long pl = (long long)P.ny * P.nz, nz = P.nz;
    const float D = fw_layer(dtab, P, i, j, k);
    const float dvx = FW_C1 * (vx[v] - fw_ld(vx, i > 0, v - pl, P.vox, 10)) - FW_C2 * (fw_ld(vx, i + 1 < P.nx, v + pl, P.vox, 10) - fw_ld(vx, i > 1, v - 2 * pl, P.vox, 10));
    const float dvy = FW_C1 * (vy[v] - fw_ld(vy, j > 0, v - nz, P.vox, 11)) - FW_C2 * (fw_ld(vy, j + 1 < P.ny, v + nz, P.vox, 11) - fw_ld(vy, j > 1, v - 2 * nz, P.vox, 11));
    const float dvz = FW_C1 * (vz[v] - fw_ld(vz, k > 0, v - 1, P.vox, 12)) - FW_C2 * (fw_ld(vz, k + 1 < P.nz, v + 1, P.vox, 12) - fw_ld(vz, k > 1, v - 2, P.vox, 12));
    const float div = dvx * P.ihx + dvy * P.ihy + dvz * P.ihz;
    const float ckp = UNI ? P.kp0 : kp[v], g = D * (UNI ? P.ga0 : ga[v]);
    const float pn = g * (p[v] - ckp * div);
    p[v] = pn;
    pmax[v] = fmaxf(pmax[v], pn);
    pmin[v] = fmaxf(pmin[v], -pn);
    if (PII) psq[v] = fmaf(pn, pn, psq[v]);
    if constexpr (LOCK) {
        float* __restrict__ lc = L.c;
        float* __restrict__ ls = L.s;
        lc[v] = fmaf(pn, L.cosf_n, lc[v]);
        ls[v] = fmaf(pn, L.sinf_n, ls[v]);
    }
}

// the split layers' arguments of the pressure launch: the component volumes, their extent and the layers' thickness
struct FwSplit { float *px, *py, *pz; long long ext; int pml; };

// d- of one axis as the gfx950 code of fullwave_pres_k rounds it: C2 (c - d) on its own, then one fused multiply-add
__device__ __forceinline__ float fw_dminus(float a, float b, float c, float d) {
#pragma clang fp contract(off)
    return fmaf(a - b, FW_C1, -(FW_C2 * (c - d)));
}

// the pressure launch of the split layers, a kernel of its own beside fullwave_pres_k (which stays as it is).  rtab is r_x | r_y | r_z.  Every rounding is
// spelled out (no contraction is left to the compiler): an interior voxel takes the roundings that the gfx950 code of fullwave_pres_k takes with D = 1 --
// div = fma(dvx, 1/h_x, dvy 1/h_y) + dvz 1/h_z, p~ = ga (p - kp div) with kp div and the difference rounded on their own -- so a run that never
// reaches a layer has the sponge's bits in the interior; a layer voxel advances its three components and does not read p.
template <bool UNI, bool PII, bool LOCK>
__global__ __launch_bounds__(FW_BLOCK) void fullwave_pres_split_k(float* __restrict__ p, const float* __restrict__ vx, const float* __restrict__ vy,
                                                                  const float* __restrict__ vz, const float* __restrict__ kp, const float* __restrict__ ga,
                                                                  const float* __restrict__ rtab, float* __restrict__ pmax, float* __restrict__ pmin,
                                                                  float* __restrict__ psq, const FullwaveParams P, const FwLock<LOCK> L, const FwSplit Q) {
#pragma clang fp contract(off)
    const long long v = (long long)blockIdx.x * FW_BLOCK + threadIdx.x;
    if (v >= P.vox || !OLX_IN(v, P.vox, 9)) return;
    int i, j, k;
    fw_ijk((unsigned)v, P, i, j, k);
    const long long pl = (long long)P.ny * P.nz, nz = P.nz;
    const float dvx = fw_dminus(vx[v], fw_ld(vx, i > 0, v - pl, P.vox, 10), fw_ld(vx, i + 1 < P.nx, v + pl, P.vox, 10), fw_ld(vx, i > 1, v - 2 * pl, P.vox, 10));
    const float dvy = fw_dminus(vy[v], fw_ld(vy, j > 0, v - nz, P.vox, 11), fw_ld(vy, j + 1 < P.ny, v + nz, P.vox, 11), fw_ld(vy, j > 1, v - 2 * nz, P.vox, 11));
    const float dvz = fw_dminus(vz[v], fw_ld(vz, k > 0, v - 1, P.vox, 12), fw_ld(vz, k + 1 < P.nz, v + 1, P.vox, 12), fw_ld(vz, k > 1, v - 2, P.vox, 12));
    const float ckp = UNI ? P.kp0 : kp[v], g = UNI ? P.ga0 : ga[v];
    float pn;
    if (i < Q.pml || i >= P.nx - Q.pml || j < Q.pml || j >= P.ny - Q.pml || k < Q.pml || k >= P.nz - Q.pml) {
        // the components live in the layer voxels only: an interior voxel never reads or writes them
        const int n = P.nx + P.ny + P.nz;
        float rx = 1.f, ry = 1.f, rz = 1.f;
        if (OLX_IN(i, n, 30) && OLX_IN(P.nx + j, n, 30) && OLX_IN(P.nx + P.ny + k, n, 30)) { rx = rtab[i]; ry = rtab[P.nx + j]; rz = rtab[P.nx + P.ny + k]; }
        float* __restrict__ qx = Q.px;
        float* __restrict__ qy = Q.py;
        float* __restrict__ qz = Q.pz;
        if (!OLX_IN(v, Q.ext, 31)) return;
        const float ax = g * (rx * (rx * qx[v] - (ckp * dvx) * P.ihx));
        const float ay = g * (ry * (ry * qy[v] - (ckp * dvy) * P.ihy));
        const float az = g * (rz * (rz * qz[v] - (ckp * dvz) * P.ihz));
        qx[v] = ax; qy[v] = ay; qz[v] = az;
        pn = (ax + ay) + az;
    } else {
        const float div = fmaf(dvx, P.ihx, dvy * P.ihy) + dvz * P.ihz;
        pn = g * (p[v] - ckp * div);
    }
    p[v] = pn;
    pmax[v] = fmaxf(pmax[v], pn);
    pmin[v] = fmaxf(pmin[v], -pn);
    if (PII) psq[v] = fmaf(pn, pn, psq[v]);
    if constexpr (LOCK) {
        float* __restrict__ lc = L.c;
        float* __restrict__ ls = L.s;
        lc[v] = fmaf(pn, L.cosf_n, lc[v]);
        ls[v] = fmaf(pn, L.sinf_n, ls[v]);
    }
}

// row n of the traces: p~ of step n at the trace voxels
__global__ void fullwave_trace_k(const float* __restrict__ p, const long long* __restrict__ pts, int npts, long long vox, float* __restrict__ row) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q < npts && OLX_IN(pts[q], vox, 13)) row[q] = p[pts[q]];
}

// the receivers of a step inside the lock-in window: row r of the CSR table is one receiver, its entries add in table order
__global__ void fullwave_receive_k(const float* __restrict__ p, const int* __restrict__ row, const long long* __restrict__ rvox, const double* __restrict__ w,
                                   int n_rec, int n_entries, long long vox, double cos_n, double sin_n, double* __restrict__ rc, double* __restrict__ rs) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rec || !OLX_IN(r + 1, n_rec + 1, 14)) return;
    double s = 0.0;
    for (int e = row[r]; e < row[r + 1]; ++e) {
        if (!OLX_IN(e, n_entries, 15)) break;
        const long long at = rvox[e];
        if (!OLX_IN(at, vox, 16)) continue;
        s = fma(w[e], (double)p[at], s);
    }
    rc[r] = fma(s, cos_n, rc[r]);
    rs[r] = fma(s, sin_n, rs[r]);
}

OLX_BOUNDS_READER(fullwave)

}  // namespace olx

using namespace olx;

static inline dim3 fw_grid(const FullwaveParams& P) { return dim3((unsigned)((P.vox + FW_BLOCK - 1) / FW_BLOCK)); }

void olx_fullwave_pack(olx_ctx* c, const float* cs, const float* rho, const float* alpha) {
    const FullwaveParams& P = c->fw;
    hipLaunchKernelGGL(fullwave_pack_k, fw_grid(P), dim3(FW_BLOCK), 0, c->stream, cs, rho, alpha, P, c->d_fw_coef[0], c->d_fw_coef[1], c->d_fw_coef[2],
                       c->d_fw_coef[3], c->d_fw_coef[4]);
}

template <bool UNI>
static void fw_launch_pres(olx_ctx* c, bool pii, bool lock, float cosf_n, float sinf_n, const float* kp, const float* ga) {
    const FullwaveParams& P = c->fw;
    const dim3 grid = fw_grid(P), block(FW_BLOCK);
    float* p = c->d_fw_p;
    const float *vx = c->d_fw_v[0], *vy = c->d_fw_v[1], *vz = c->d_fw_v[2], *dtab = c->d_fw_dtab;
    float *pmax = c->d_fw_pmax, *pmin = c->d_fw_pmin, *psq = pii ? (float*)c->d_fw_psq : nullptr;
    const FwLock<true> L{c->d_fw_lc, c->d_fw_ls, cosf_n, sinf_n};
    if (lock) {
        if (pii) hipLaunchKernelGGL((fullwave_pres_k<UNI, true, true>), grid, block, 0, c->stream, p, vx, vy, vz, kp, ga, dtab, pmax, pmin, psq, P, L);
        else hipLaunchKernelGGL((fullwave_pres_k<UNI, false, true>), grid, block, 0, c->stream, p, vx, vy, vz, kp, ga, dtab, pmax, pmin, psq, P, L);
    } else {
        if (pii) hipLaunchKernelGGL((fullwave_pres_k<UNI, true, false>), grid, block, 0, c->stream, p, vx, vy, vz, kp, ga, dtab, pmax, pmin, psq, P, FwLock<false>{});
        else hipLaunchKernelGGL((fullwave_pres_k<UNI, false, false>), grid, block, 0, c->stream, p, vx, vy, vz, kp, ga, dtab, pmax, pmin, psq, P, FwLock<false>{});
    }
}

template <bool UNI>
static void fw_launch_pres_split(olx_ctx* c, bool pii, bool lock, float cosf_n, float sinf_n, const float* kp, const float* ga) {
    const FullwaveParams& P = c->fw;
    const dim3 grid = fw_grid(P), block(FW_BLOCK);
    float* p = c->d_fw_p;
    const float *vx = c->d_fw_v[0], *vy = c->d_fw_v[1], *vz = c->d_fw_v[2], *rtab = c->d_fw_rtab;
    float *pmax = c->d_fw_pmax, *pmin = c->d_fw_pmin, *psq = pii ? (float*)c->d_fw_psq : nullptr;
    const FwLock<true> L{c->d_fw_lc, c->d_fw_ls, cosf_n, sinf_n};
    long long ext = (long long)c->d_fw_pc[0].capacity();
    for (const DevBuf<float>& b : c->d_fw_pc) ext = std::min(ext, (long long)b.capacity());
    const FwSplit Q{c->d_fw_pc[0], c->d_fw_pc[1], c->d_fw_pc[2], ext, c->fw_pml};
    if (lock) {
        if (pii) hipLaunchKernelGGL((fullwave_pres_split_k<UNI, true, true>), grid, block, 0, c->stream, p, vx, vy, vz, kp, ga, rtab, pmax, pmin, psq, P, L, Q);
        else hipLaunchKernelGGL((fullwave_pres_split_k<UNI, false, true>), grid, block, 0, c->stream, p, vx, vy, vz, kp, ga, rtab, pmax, pmin, psq, P, L, Q);
    } else {
        if (pii) hipLaunchKernelGGL((fullwave_pres_split_k<UNI, true, false>), grid, block, 0, c->stream, p, vx, vy, vz, kp, ga, rtab, pmax, pmin, psq, P, FwLock<false>{}, Q);
        else hipLaunchKernelGGL((fullwave_pres_split_k<UNI, false, false>), grid, block, 0, c->stream, p, vx, vy, vz, kp, ga, rtab, pmax, pmin, psq, P, FwLock<false>{}, Q);
    }
}

void olx_fullwave_step(olx_ctx* c, int step, bool pii) {
    const FullwaveParams& P = c->fw;
    const FullwaveSource& S = c->fw_src;
    float* p = c->d_fw_p;
    if (S.n_vox > 0 && c->fw_elem)
        hipLaunchKernelGGL(fullwave_inject_elem_k, dim3((S.n_vox + 63) / 64), dim3(64), 0, c->stream, p, c->d_fw_svox, c->d_fw_srow, c->d_fw_samp, c->d_fw_sel,
                           c->d_fw_drive, S.n_vox, c->fw_entries, c->fw_nel, (long long)c->fw_steps * c->fw_nel, P.vox, step);
    else if (S.n_vox > 0)
        hipLaunchKernelGGL(fullwave_inject_k, dim3((S.n_vox + 63) / 64), dim3(64), 0, c->stream, p, c->d_fw_svox, c->d_fw_srow, c->d_fw_samp, c->d_fw_stau, S,
                           c->fw_entries, P.vox, step);
    const dim3 grid = fw_grid(P), block(FW_BLOCK);
    float *vx = c->d_fw_v[0], *vy = c->d_fw_v[1], *vz = c->d_fw_v[2];
    const bool split = c->fw_layers == 1;
    const float* dtab = split ? c->d_fw_stab : c->d_fw_dtab;
    // the lock-in of a step inside the window: theta_n = 2 pi frac(f0 t_n), t_n = (n + 1) dt, in fp64
    const bool lock = c->fw_lock && step >= c->fw_lock_w0 && step < c->fw_lock_w0 + c->fw_lock_nw;
    double cos_n = 0.0, sin_n = 0.0;
    if (lock) {
        double ph = c->fw_lock_freq * ((double)(step + 1) * c->fw_dt);
        ph -= std::floor(ph);
        cos_n = std::cos(2.0 * M_PI * ph); sin_n = std::sin(2.0 * M_PI * ph);
    }
    const bool lock_vol = lock && c->fw_lock_vol;
    if (c->fw_uniform) {
        if (split) {
            hipLaunchKernelGGL((fullwave_vel_k<true, true>), grid, block, 0, c->stream, p, vx, vy, vz, nullptr, nullptr, nullptr, dtab, P);
            fw_launch_pres_split<true>(c, pii, lock_vol, (float)cos_n, (float)sin_n, nullptr, nullptr);
        } else {
            hipLaunchKernelGGL(fullwave_vel_k<true>, grid, block, 0, c->stream, p, vx, vy, vz, nullptr, nullptr, nullptr, dtab, P);
            fw_launch_pres<true>(c, pii, lock_vol, (float)cos_n, (float)sin_n, nullptr, nullptr);
        }
    } else {
        const float *bx = c->d_fw_coef[0], *by = c->d_fw_coef[1], *bz = c->d_fw_coef[2], *kp = c->d_fw_coef[3], *ga = c->d_fw_coef[4];
        if (split) {
            hipLaunchKernelGGL((fullwave_vel_k<false, true>), grid, block, 0, c->stream, p, vx, vy, vz, bx, by, bz, dtab, P);
            fw_launch_pres_split<false>(c, pii, lock_vol, (float)cos_n, (float)sin_n, kp, ga);
        } else {
            hipLaunchKernelGGL(fullwave_vel_k<false>, grid, block, 0, c->stream, p, vx, vy, vz, bx, by, bz, dtab, P);
            fw_launch_pres<false>(c, pii, lock_vol, (float)cos_n, (float)sin_n, kp, ga);
        }
    }
    if (c->fw_npts > 0)
        hipLaunchKernelGGL(fullwave_trace_k, dim3((c->fw_npts + 255) / 256), dim3(256), 0, c->stream, p, c->d_fw_pts, c->fw_npts, P.vox,
                           c->d_fw_trace + (size_t)step * c->fw_npts);
    if (lock && c->fw_lock_nrec > 0)
        hipLaunchKernelGGL(fullwave_receive_k, dim3((c->fw_lock_nrec + 63) / 64), dim3(64), 0, c->stream, p, c->d_fw_lrow, c->d_fw_lvox, c->d_fw_lw,
                           c->fw_lock_nrec, c->fw_lock_entries, P.vox, cos_n, sin_n, c->d_fw_lrc, c->d_fw_lrs);
}

void olx_fullwave_aperture_weights(olx_ctx* c, int n_el, long long max_box, long long total) {
    hipLaunchKernelGGL(fullwave_aperture_k, dim3((unsigned)n_el, (unsigned)((max_box + FW_BLOCK - 1) / FW_BLOCK)), dim3(FW_BLOCK), 0, c->stream, c->d_fw_ap, n_el,
                       c->fw_origin[0], c->fw_origin[1], c->fw_origin[2], c->fw_h[0], c->fw_h[1], c->fw_h[2], c->d_fw_apw, total);
}

void olx_fullwave_drive_fill(olx_ctx* c) {
    const long long total = (long long)c->fw_steps * c->fw_nel;
    if (c->fw_drive_mode != 1) {
        hipLaunchKernelGGL(fullwave_drive_k, dim3((unsigned)((total + FW_BLOCK - 1) / FW_BLOCK)), dim3(FW_BLOCK), 0, c->stream, c->d_fw_dA, c->d_fw_dtau, c->fw_src,
                           c->fw_nel, total, 0ll, (long long)c->fw_nel, 1ll, c->d_fw_drive);
        return;
    }
    // the response drive: the bare burst of the steps -(M_max - 1) .. n_steps - 1, element-major, then the classes' taps over it
    const int lead = c->fw_resp_mmax - 1;
    const long long rows = (long long)c->fw_steps + lead, ext = rows * c->fw_nel;
    hipLaunchKernelGGL(fullwave_drive_k, dim3((unsigned)((ext + FW_BLOCK - 1) / FW_BLOCK)), dim3(FW_BLOCK), 0, c->stream, c->d_fw_dA, c->d_fw_dtau, c->fw_src,
                       c->fw_nel, ext, -(long long)lead, 1ll, rows, c->d_fw_dext);
    const long long chunks = ((long long)c->fw_steps + FW_BLOCK - 1) / FW_BLOCK;
    hipLaunchKernelGGL(fullwave_drive_fir_k, dim3((unsigned)(chunks * c->fw_nel)), dim3(FW_BLOCK), 0, c->stream, c->d_fw_dext, c->d_fw_gcls, c->d_fw_grow,
                       c->d_fw_gtaps, c->fw_nel, c->fw_resp_classes, c->fw_resp_ntaps, c->fw_steps, lead, c->d_fw_drive);
}
