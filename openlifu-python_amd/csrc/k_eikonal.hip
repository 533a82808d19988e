// kernel 6 (eikonal_init_k, eikonal_sweep_k, eikonal_sample_k): first-arrival travel times from a point through a heterogeneous sound speed --
// the first-order upwind (Godunov) eikonal update, swept Jacobi-wise until a sweep changes nothing.  gfx950 (CDNA4, wave64) only.
// Definition: DESIGN.md section 2 ("Eikonal") and section 5.17, fp64 oracle tests/eikonal_oracle.py.
//
// T lives at voxel centres (C order, z fastest), fp32, in two ping-pong buffers; +inf = nothing has arrived.  Slowness s(v) = 1 / c(v),
// formed in ONE place (ek_slowness) for the uniform (UNI, no volume streamed) and the volume instantiation: a volume filled with the
// uniform value gives the same bits.
//   init    voxels within init_radius (index space, fp64 test) of the source get T = |x_v - x_t| s(v) in BOTH buffers and are frozen;
//           every other voxel +inf
//   sweep   reads T_in, writes T_out, one lane per voxel of the launch box: m_a = min of the two neighbours along axis a (+inf outside
//           the grid), the three (m_a, h_a) sorted by m (stable), t = a1 + s h1, then the two- and the three-axis quadratic written
//           relative to a1 while the next a_i is below t; T_out = min(T_in, t).  A block with a lane that lowered its voxel stores 1
//           into the sweep's own flag (zeroed before the solve; the host reads the flags every few sweeps).
//           The launch box is the init box grown by one voxel per sweep, clipped by the grid: a voxel outside it has only +inf
//           neighbours and stays +inf, in both buffers.
//   sample  T at points: ONE thread per point walks its CSR row, sum_q w_q (double) T(vox_q) in table order (fullwave_receive_k's form)
#include "k_types.hip.h"
#include "olx_ctx.h"
#include "olx_launch.h"

namespace olx {

constexpr int EK_BLOCK = 256;

// the slowness of voxel v: the one place it is formed
template <bool UNI> __device__ __forceinline__ float ek_slowness(const float* __restrict__ cs, const EikonalParams& P, long long v) {
    const float c = UNI ? P.c0 : cs[v];
    return __builtin_amdgcn_rcpf(c);          // v_rcp_f32 (1 ulp): the same instruction for both instantiations
}

// the frozen test of the init set: index-space distance of voxel (i, j, k) from the source in fp64, evaluated inside the host's init box only
__device__ __forceinline__ bool ek_frozen(const EikonalParams& P, int i, int j, int k) {
    if (i < P.ilo[0] || i > P.ihi[0] || j < P.ilo[1] || j > P.ihi[1] || k < P.ilo[2] || k > P.ihi[2]) return false;
    const double di = (double)i - P.q[0], dj = (double)j - P.q[1], dk = (double)k - P.q[2];
    return sqrt(di * di + dj * dj + dk * dk) <= P.radius;
}

template <bool UNI>
__global__ __launch_bounds__(EK_BLOCK) void eikonal_init_k(float* __restrict__ t0, float* __restrict__ t1, const float* __restrict__ cs, const EikonalParams P) {
    const long long v = (long long)blockIdx.x * EK_BLOCK + threadIdx.x;
    if (v >= P.vox || !OLX_IN(v, P.vox, 0)) return;
    const unsigned row = (unsigned)v / (unsigned)P.nz;
    const int k = (int)((unsigned)v - row * (unsigned)P.nz), i = (int)(row / (unsigned)P.ny), j = (int)(row - (unsigned)i * (unsigned)P.ny);
    float t = __builtin_huge_valf();
    if (ek_frozen(P, i, j, k)) {
        const double dx = ((double)i - P.q[0]) * P.h[0], dy = ((double)j - P.q[1]) * P.h[1], dz = ((double)k - P.q[2]) * P.h[2];
        t = (float)(sqrt(dx * dx + dy * dy + dz * dz) * (double)ek_slowness<UNI>(cs, P, v));
    }
    t0[v] = t;
    t1[v] = t;
}

// T_in[u] when the neighbour is inside the grid by the caller's index test (checked against the extent in the debug library), +inf otherwise
__device__ __forceinline__ float ek_ld(const float* __restrict__ a, bool inside, long long u, long long vox, int site) {
    return (inside && OLX_IN(u, vox, site)) ? a[u] : __builtin_huge_valf();
}

// x = (B + sqrt(max(B^2 - A C, 0))) / A: the larger root of A x^2 - 2 B x + C = 0
// (v_sqrt_f32 and v_rcp_f32, 1 ulp each: the operands are O(1) here, far from the denormals, and the sweep is bound by its instructions)
__device__ __forceinline__ float ek_root(float A, float B, float C) { return (B + __builtin_amdgcn_sqrtf(fmaxf(B * B - A * C, 0.f))) * __builtin_amdgcn_rcpf(A); }

// l / d for l < 2^31 by the multiplier m = ceil(2^(31 + s) / d), s = ceil(log2 d) (EikonalBox, formed on the host): exact
__device__ __forceinline__ unsigned ek_div(unsigned l, unsigned m, int sh) { return (unsigned)(((unsigned long long)l * m) >> sh); }

template <bool UNI>
__global__ __launch_bounds__(EK_BLOCK) void eikonal_sweep_k(const float* __restrict__ tin, float* __restrict__ tout, const float* __restrict__ cs,
                                                            const EikonalParams P, const EikonalBox B, int* __restrict__ flag) {
    const long long l = (long long)blockIdx.x * EK_BLOCK + threadIdx.x;
    bool lowered = false;
    if (l < B.count) {
        // (i, j, k) of box lane l, z fastest (count < 2^31: two exact multiply-shift divisions)
        const unsigned row = ek_div((unsigned)l, B.mul[2], B.sh[2]);
        const int bk = (int)((unsigned)l - row * (unsigned)B.n[2]), bi = (int)ek_div(row, B.mul[1], B.sh[1]), bj = (int)(row - (unsigned)bi * (unsigned)B.n[1]);
        const int i = B.lo[0] + bi, j = B.lo[1] + bj, k = B.lo[2] + bk;
        const long long pl = (long long)P.ny * P.nz, nz = P.nz;
        const long long v = ((long long)i * P.ny + j) * nz + k;
        if (OLX_IN(v, P.vox, 1)) {
            const float tc = tin[v];
            float t = tc;
            if (!ek_frozen(P, i, j, k)) {
                const float s = ek_slowness<UNI>(cs, P, v);
                float m0 = fminf(ek_ld(tin, i > 0, v - pl, P.vox, 2), ek_ld(tin, i + 1 < P.nx, v + pl, P.vox, 2));
                float m1 = fminf(ek_ld(tin, j > 0, v - nz, P.vox, 3), ek_ld(tin, j + 1 < P.ny, v + nz, P.vox, 3));
                float m2 = fminf(ek_ld(tin, k > 0, v - 1, P.vox, 4), ek_ld(tin, k + 1 < P.nz, v + 1, P.vox, 4));
                float h0 = P.hf[0], h1 = P.hf[1], h2 = P.hf[2], w0 = P.wf[0], w1 = P.wf[1], w2 = P.wf[2];
                // ascending by m, ties in axis order (three strict compare-exchanges of neighbours: stable)
                auto cx = [](float& ma, float& ha, float& wa, float& mb, float& hb, float& wb) {
                    if (mb < ma) { float x = ma; ma = mb; mb = x; x = ha; ha = hb; hb = x; x = wa; wa = wb; wb = x; }
                };
                cx(m0, h0, w0, m1, h1, w1);
                cx(m1, h1, w1, m2, h2, w2);
                cx(m0, h0, w0, m1, h1, w1);
                float tn = m0 + s * h0;
                if (m1 < tn) {
                    const float u1 = m1 - m0;
                    float A = w0 + w1, Bq = w1 * u1, C = w1 * u1 * u1 - s * s;
                    tn = m0 + ek_root(A, Bq, C);
                    if (m2 < tn) {
                        const float u2 = m2 - m0;
                        A = w0 + w1 + w2; Bq = w1 * u1 + w2 * u2; C = w1 * u1 * u1 + w2 * u2 * u2 - s * s;
                        tn = m0 + ek_root(A, Bq, C);
                    }
                }
                t = fminf(tc, tn);
                lowered = t < tc;
            }
            tout[v] = t;
        }
    }
    if (__syncthreads_or(lowered) && threadIdx.x == 0) *flag = 1;
}

// T at the points: row r of the CSR table is one point, its entries add in table order
__global__ void eikonal_sample_k(const float* __restrict__ t, const int* __restrict__ row, const long long* __restrict__ pvox, const double* __restrict__ w,
                                 int n_points, int n_entries, long long vox, double* __restrict__ out) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_points || !OLX_IN(r + 1, n_points + 1, 5)) return;
    double s = 0.0;
    for (int e = row[r]; e < row[r + 1]; ++e) {
        if (!OLX_IN(e, n_entries, 6)) break;
        const long long at = pvox[e];
        if (!OLX_IN(at, vox, 7)) continue;
        s = fma(w[e], (double)t[at], s);
    }
    out[r] = s;
}

OLX_BOUNDS_READER(eikonal)

}  // namespace olx

using namespace olx;

void olx_eikonal_init(olx_ctx* c, const float* cs) {
    const EikonalParams& P = c->ek;
    const dim3 grid((unsigned)((P.vox + EK_BLOCK - 1) / EK_BLOCK)), block(EK_BLOCK);
    if (cs) hipLaunchKernelGGL(eikonal_init_k<false>, grid, block, 0, c->stream, c->d_ek_T[0], c->d_ek_T[1], cs, P);
    else hipLaunchKernelGGL(eikonal_init_k<true>, grid, block, 0, c->stream, c->d_ek_T[0], c->d_ek_T[1], cs, P);
}

void olx_eikonal_sweep(olx_ctx* c, const float* cs, int sweep) {
    const EikonalParams& P = c->ek;
    // sweep number `sweep` (from 1) reads buffer (sweep - 1) & 1 and writes the other, over the init box grown by `sweep` voxels
    EikonalBox B;
    const int n[3] = {P.nx, P.ny, P.nz};
    B.count = 1;
    for (int a = 0; a < 3; ++a) {
        const long long lo = std::max((long long)P.ilo[a] - sweep, 0ll), hi = std::min((long long)P.ihi[a] + sweep, (long long)n[a] - 1);
        B.lo[a] = (int)lo; B.n[a] = (int)(hi - lo + 1);
        B.count *= B.n[a];
        int sh = 0;
        while ((1u << sh) < (unsigned)B.n[a]) ++sh;
        B.sh[a] = 31 + sh;
        B.mul[a] = (unsigned)(((1ull << B.sh[a]) + (unsigned)B.n[a] - 1) / (unsigned)B.n[a]);
    }
    const float* tin = c->d_ek_T[(sweep - 1) & 1];
    float* tout = c->d_ek_T[sweep & 1];
    const dim3 grid((unsigned)((B.count + EK_BLOCK - 1) / EK_BLOCK)), block(EK_BLOCK);
    int* flag = c->d_ek_flag + (sweep - 1);
    if (cs) hipLaunchKernelGGL(eikonal_sweep_k<false>, grid, block, 0, c->stream, tin, tout, cs, P, B, flag);
    else hipLaunchKernelGGL(eikonal_sweep_k<true>, grid, block, 0, c->stream, tin, tout, cs, P, B, flag);
}

void olx_eikonal_sample_launch(olx_ctx* c, int n_points, int n_entries) {
    hipLaunchKernelGGL(eikonal_sample_k, dim3((n_points + 63) / 64), dim3(64), 0, c->stream, c->d_ek_T[c->ek_cur], c->d_ek_row, c->d_ek_vox, c->d_ek_w,
                       n_points, n_entries, c->ek.vox, c->d_ek_out);
}
