// kernel 2g (field_cosetp_k): kernel 2e's NT = 2 shape with the PLANES in the MFMA rows -- no output staging
// gfx950 (CDNA4, wave64) only.  Data layout in HBM: DESIGN.md section 4; launchers declared in olx_launch.h.
#include <algorithm>
#include <cstdlib>
#include "k_types.hip.h"
#include "olx_ctx.h"
#include "olx_launch.h"

namespace olx {

// ------------------------------------------------------------------------------------
// Kernel 2e gives a wave a position grid on 2 planes and lists (plane, position) down the MFMA rows; its results then sit
// in registers with the z neighbours of a voxel in OTHER waves, so every block transposes its whole output through LDS
// (|p| -> staging -> barrier -> read-out over a job list -> 64-byte runs): 29 % of a wave's lifetime on the headline shard.
// Here the block's footprint, operands, tables and arithmetic are the same, but the row map is turned:
//   * MFMA tile = ONE position x the block's 16 planes (row = plane).  Wave w takes the positions w, w + 8, ... of the
//     block's position grid (<= 5 tiles).  A lane then holds, for its column, rows 4 g .. 4 g + 3 = FOUR CONSECUTIVE PLANES
//     of one voxel column: |p| / intensity in place, one 16-byte store per store target straight from the accumulators
//     (after one lane transpose four CONSECUTIVE lanes write 64 contiguous bytes, as kernel 2e's read-out does).
//     No staging arena, no epilogue barriers, no job-list pass.
//   * The geometry tables of the 16 planes are shared by the block: wave w still evaluates planes 2 w, 2 w + 1 (same
//     26-row pair tables, same arithmetic), behind the block barriers that the steering-fragment staging needs anyway.
//   * A fragment of row p (plane), k-group g: table of plane p, row ky - g + ROW0 - 4 kb - 8 sl, entries UW - 8 - 2 kx + 4 ka ..:
//     a per-lane base (plane, g) + a wave-uniform tile offset.  Plane stride 364 words (182 = 22 (mod 32) 8-byte slots: 16 planes ->
//     16 distinct even slots) and row stride 14 words (7 slots: the second k-group of a ds_read_b64 lane group -> the odd slots)
//     put the 32 lanes of a ds_read_b64 group (16 planes x 2 k-groups) on 32 distinct 8-byte slots.
//   * Table pairs (sa - 1, sbb0) and (sa, sbb0) of a block cover the columns [-7 - 8 (sa - 1), 4 - 8 (sa - 1)] and 8 further left: they
//     share 4 of 12 (same integer U, dx, row and plane: the same bits).  Where a pair follows its left neighbour directly (nsbp == 2: every
//     16-row array) each wave MOVES words 8 .. 11 of its own planes' rows to words 0 .. 3 and evaluates only the 8 new columns on an
//     8 columns x 8 rows lane map: 7 instead of 11 evaluations per lane for that pair (OLX_EXP_CP_NOREUSE=1 in developer builds: A/B).
//   * |p| alone (what the product launches since the intensity is derived from |p|) is an instantiation of its own: PONLY -- no intensity
//     values, 4 instead of 8 ds_bpermute per position, no flag test at the stores.
// NT = 2 (9 - 16 distinct steering columns), KX <= 3: the shape of BASELINE's 8-focus shard; the other shapes stay with 2e.
// Measured on the headline shard (8 foci, 256 el x 256^3, alternating runs on one box): 0.404 vs 0.430 ms with fp8 corrections,
// 0.456 vs 0.499 ms with fp16 corrections (kernel 2e).  A first version was 12 % SLOWER: the read-out loop carried the ragged-nz
// store form in the same body, which makes the compiler split every 16-byte store into 12 + 4 bytes (twice the store
// instructions, and the vector memory pipe takes ~16 cycles per wave-instruction whatever its width or exec mask).
// ------------------------------------------------------------------------------------
constexpr int CP_TW = 14;                          // words per table row (12 in use): = 2 (mod 4)
constexpr int CP_TROWS = 26, CP_ROW0 = 15;         // pair table rows; row of offset wd = 0
constexpr int CP_PSZ = 364;                        // words per plane table = 26 x 14; PSZ / 2 = 22 (mod 32): see above
constexpr int CP_UW = 12;                          // table columns: ud = 2 kx - a in [-7, 4]
constexpr int CP_SHARED = 4;                       // columns a pair (sa, sbb0) shares with (sa - 1, sbb0): [-7 - 8 sa, 4 - 8 sa] and its neighbour overlap in 4
constexpr int CP_MT = 5;                           // tiles (positions) per wave: ceil(33 / 8)
constexpr int CP_AHEAD_N = 7;                      // evaluations per lane of a reuse-form fill: the words a wave holds when it fills ahead

#ifdef OLX_EXP_CUTRACE
// developer build only (tools/cutrace_cosetp.py): per block and wave {HW_ID, XCC_ID, cycle at entry, at the last store issued, at the
// last store acknowledged} -- the occupancy timeline of a CU (how long a slot idles between two blocks)
static __device__ unsigned long long g_cutrace[16384][8][5];
#define OLX_CUTRACE(k, v) do { if (lane == 0 && blockIdx.y == 0 && blockIdx.x < 16384) g_cutrace[blockIdx.x][wave][k] = (v); } while (0)
#else
#define OLX_CUTRACE(k, v)
#endif

template <int MX, int MY, bool CLAMP, bool FP8, bool DIR = false, bool BOTH = true /*|p| and intensity both wanted: no flag tests between the stores*/,
          bool PONLY = false /*|p| alone (the product's case since the intensity is derived): no intensity arithmetic, lane exchange or flag test*/>
__global__ __launch_bounds__(COS_NW * 64, 4) void field_cosetp_k(
    const uint4* __restrict__ bfrag, float* __restrict__ pmag, float* __restrict__ inten,
    const int* __restrict__ targets /*[tiles][32 columns][4]: focus * 4 + mirror image, -1 = none*/,
    const CosetBlock* __restrict__ blocks /*[n_items]*/, const CosetParams P) {
    constexpr int NT = 2, THREADS = COS_NW * 64, PAIR = 2;
    // fill-ahead (below), per instantiation by measurement: the fp8 shape (the headline) has it; with fp16 corrections and in the DIR instantiations the
    // matrix pipe is the scarcer unit and the reuse fill stays a phase of its own
    constexpr bool AHEAD = FP8;
    constexpr bool PRE_LATE = AHEAD;             // the next pair's steering fragments are requested behind the K-steps instead of in front of them (below)
    static_assert(!(BOTH && PONLY), "one output or both");
    constexpr int TROWS = CP_TROWS, ROW0 = CP_ROW0, PSZ = CP_PSZ, MT = CP_MT;   // 26-row pair tables, 364 words per plane, <= 5 tiles per wave
    static_assert((PSZ / 2) % 2 == 0 && ((PSZ / 2) % 32 == 22 || (PSZ / 2) % 32 == 30), "16 planes on 16 distinct even 8-byte slots");
    constexpr int B_KS_U4 = 128;                                                // uint4 per K-step and column tile: hi, lo (64 lanes each)
    constexpr int B_BYTES = PAIR * 4 * NT * B_KS_U4 * 16;                       // PAIR super-blocks of steering fragments
    constexpr int T_WORDS = COS_ZB * PSZ;
    __shared__ __attribute__((aligned(16))) unsigned char smem[B_BYTES + T_WORDS * 4 + T_WORDS * 4 + 64];
    // steering stage: K-step record (sl * 4 + ks, nt) = B_KS_U4 uint4: [0] hi, [1] lo of the 64 lanes
    auto s_B = [&](int rec, int nt, int part) -> const uint4* { return reinterpret_cast<const uint4*>(smem) + ((size_t)(rec * NT + nt) * B_KS_U4 + part * 64); };
    unsigned* const s_hi = reinterpret_cast<unsigned*>(smem + B_BYTES);
    unsigned* const s_lo = s_hi + T_WORDS;
    const int tile = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, p16 = lane & 15;
    OLX_CUTRACE(2, __builtin_readcyclecounter());
    OLX_CUTRACE(0, (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4));      // HW_REG_HW_ID
    OLX_CUTRACE(1, (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20));     // HW_REG_XCC_ID
    // the block's share of the coset decomposition: one scalar load of the host's record (olx.hip; blockIdx order as in kernel 2e,
    // the two blocks that write the two 64-byte halves of the same 128-byte lines 8 ids apart = same XCD).  Decoded here it was
    // ~350 VALU instructions per wave -- a fifth of the wave's vector instructions: integer divisions have no scalar form.
    const int item = blockIdx.x;
    {
    const CosetBlock BK = blocks[item];
    const int npos = BK.npos, KY = BK.KY, ky_magic = BK.ky_magic;
    if (npos <= 0) return;                              // block-uniform
    const int ibase = BK.ibase, jbase = BK.jbase;
    const int k0 = BK.k0;
    // (Wave 0 always holds the extra tile of a 33-position block, but the dispatcher starts a block's waves on a different SIMD from block to block: over a
    // launch every SIMD of a CU carries the same number of tiles as it is.  Rotating the ownership per record made the launch 1.4 % slower: DESIGN 5.6.)
    const int ntile = __builtin_amdgcn_readfirstlane((npos - wave + COS_NW - 1) / COS_NW);      // this wave's positions: wave, wave + 8, ... (wave-uniform, <= MT)
    // table generation role (planes 2 wave, 2 wave + 1): full form lane -> (wl = lane / 12 < 5, ui = lane % 12), round r: rows 5 r + wl; reuse form 8 x 8 (the fill lambda below).
    // (Its per-lane constants are formed inside the pair loop from an opaque copy of the lane index: hoisted, they would be live
    // across the K-steps, where the fp8 shape has no register to spare -- 5 spilled registers cost 190 MB of scratch traffic.)
    // fragment read offset [words] of a tile's row for K-step (0, 0) = per-lane part (plane, k-group) + the tile's position (wave-uniform)
    const int lane_off = p16 * PSZ - g * CP_TW;
    int toff[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        const int pos = min(wave + COS_NW * t, npos - 1);
        const int kx = (pos * ky_magic) >> 16, ky = pos - kx * KY;                // scalar: pos / KY, exact for pos <= 40 (host checks)
        toff[t] = (ky + ROW0) * CP_TW + (CP_UW - 8 - 2 * kx);
    }
    // A tile-step (one tile in one (sl, kb) group) issues no vector instruction but its matrix instructions -- inside the K-steps every other one takes an issue
    // slot from the matrix instructions of the SIMD's other waves.  The byte addresses of the wave's <= 5 tiles are formed here, once per block, and
    // held across the pairs (opaque: neither re-derived nor sunk into the tile-steps); every fragment read takes its K-step and array offset as an immediate.
    // Five registers: the e4m3 K-steps leave 21 since PRE_LATE (118 VGPRs with the clamp), the other instantiations have 94.
    unsigned frag_b[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        frag_b[t] = (unsigned)(lane_off + toff[t]) << 2;
        asm volatile("" : "+v"(frag_b[t]));
    }
    // ... and the wave-uniform tile guards `t >= ntile` compare an SGPR copy of the tile count that every group of tile-steps takes for itself: shared by all
    // groups, the compiler kept the four conditions as lane masks and passed them through a v_cndmask / v_cmp pair per tile
    auto tile_count = [&]() __attribute__((always_inline)) {
        int n = ntile;
        asm volatile("" : "+s"(n));
        return n;
    };
    // fragment words of tile t at word offset kso from its K-step (0, 0) position in table array `arr`
    auto frag_at = [&](const unsigned* const arr, const int t, const int kso) __attribute__((always_inline)) -> const unsigned long long* {
        return reinterpret_cast<const unsigned long long*>(reinterpret_cast<const unsigned char*>(arr + kso) + frag_b[t]);
    };
    floatx4_t acc[MT][NT];
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[t][nt] = floatx4_t{0.f, 0.f, 0.f, 0.f};
    const int nsbp = P.nsbp;                    // even: chunks = table pairs never straddle sa
    const int n_sb = P.nsa * nsbp;
    bool reuse_ok = nsbp == PAIR;
#ifdef OLX_DEV_PINS
    reuse_ok = reuse_ok && P.cp_noreuse == 0;   // OLX_EXP_CP_NOREUSE=1 (A/B): every pair takes the full fill
#endif
    // fill-ahead: a pair that will take the reuse form has its 7 evaluations per lane done in front of the K-steps of the pair before it, behind the
    // barrier that opens them; the 14 words wait in registers for the barrier that frees the table, and the fill phase between that barrier and the
    // next shrinks to the 4-column move and 14 LDS writes per lane
    bool ahead_ok = AHEAD && reuse_ok;          // (block-uniform)
#ifdef OLX_DEV_PINS
    ahead_ok = ahead_ok && P.cp_nofillahead == 0;   // OLX_EXP_CP_NOFILLAHEAD=1 (A/B): the reuse fill stays a phase of its own (PRE_LATE is a compile-time choice and stays)
#endif
    const bool my_planes = k0 + wave * COS_P < P.nz;      // (wave-uniform) a wave whose planes lie beyond nz fills, moves and evaluates nothing
    unsigned held_hi[CP_AHEAD_N], held_lo[CP_AHEAD_N];     // written and read under the same wave-uniform condition
    // dz^2 of plane z of this wave (opaque: every use adds the same rounded square, never a fused dz * dz + r2)
    auto plane_dz2 = [&](const int z) __attribute__((always_inline)) {
        const float dz = (float)(k0 + wave * COS_P + z) * P.hz - P.flat_ez;
        float q = dz * dz;
        if constexpr (AHEAD) asm volatile("" : "+v"(q));      // (only where two code paths evaluate the same entries: the others keep their code as it was)
        return q;
    };
    // one table entry: G of squared lateral distance r2 on a plane dz2v above the elements -> hi / lo words
    auto entry = [&](const float r2, const float dz2v, const float dx, const float dy, unsigned& hi_word, unsigned& lo_word) __attribute__((always_inline)) {
        float d2 = r2 + dz2v;
        if (CLAMP) d2 = fmaxf(d2, P.dmin2);
        const float ri = __builtin_amdgcn_rsqf(d2);
        const float ph = d2 * ri;
        float rs = ri * P.g_scale;
        if constexpr (DIR) rs *= table_mod(dx, dy, ph, ri, P.dir_wx, P.dir_wy, P.absorb_l2);      // (own instantiations: the default path never sees this)
        float gr = rs * __builtin_amdgcn_cosf(ph), gi = rs * __builtin_amdgcn_sinf(ph);
        asm volatile("" : "+v"(gr), "+v"(gi));      // (two plain multiplies: packed fp32 beside the partner block's matrix instructions measured slower)
        half2_t hi;
        if constexpr (FP8) hi = __builtin_convertvector(float2_t{gr, gi}, half2_t);      // to nearest: |lo| <= half an ulp
        else hi = __builtin_bit_cast(half2_t, __builtin_amdgcn_cvt_pkrtz(gr, gi));
        // lo = g - (float)hi in ONE mixed-precision fma per component (the compiler's form: a convert and a subtract)
        float lr, li;
        const unsigned hw = __builtin_bit_cast(unsigned, hi);
        asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(lr) : "v"(hw), "v"(gr));
        asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(li) : "v"(hw), "v"(gi));
        if constexpr (FP8) {             // e4m3 bytes [lo re, lo im | hi re, hi im], |.| <= 256 (448 overflows to NaN)
            // (v_cvt_scalef32_pk_fp8_f32 DIVIDES by its power-of-two scale operand -- tools/probe/cvt_scale_probe.hip --
            // and rounds / saturates as the unscaled convert: the four operand scalings cost no instruction)
            short2_t w;                  // (both halves are written below)
            w = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(w, lr, li, 1.0f / COS_F8_LO, false);
            w = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(w, gr, gi, 1.0f / COS_F8_HI, true);
            lo_word = __builtin_bit_cast(unsigned, w);
        } else {
            lo_word = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(lr, li));
        }
        hi_word = hw;
    };
    auto put = [&](const int o, const bool ok, const unsigned hi_word, const unsigned lo_word) __attribute__((always_inline)) {
        if (ok && OLX_IN(o, T_WORDS, 0)) {
            s_hi[o] = hi_word;
            s_lo[o] = lo_word;
        }
    };
    // The REUSE form of the pair (sa_f, sbb_f) on the 8 columns x 8 rows lane map (the fill lambda below, RU), entry by entry: e = 2 r + z for round r,
    // plane z; e = 6 the tail rows.  The per-lane constants are formed where these are called, from an opaque copy of the lane index: nothing of them
    // lives across the tiles.  ru_slot: the table offset of entry e and whether the lane's entry exists; ru_eval_all: the words of all entries.
    constexpr int RU_CW = CP_UW - CP_SHARED, RU_ROWS = 64 / RU_CW, RU_NR = (CP_TROWS - COS_P) / RU_ROWS;
    static_assert(CP_AHEAD_N == RU_NR * COS_P + 1 && RU_CW == 8 && RU_ROWS == 8 && COS_P == 2, "the reuse form: 3 rounds x 2 planes and the tail rows");
    auto ru_slot = [&](const int e, const int lane_o, int& o, bool& ok) __attribute__((always_inline)) {
        const int wl = lane_o >> 3, ui = lane_o & 7;
        if (e < RU_NR * COS_P) {
            o = (wave * COS_P + (e & 1)) * PSZ + (wl + RU_ROWS * (e >> 1)) * CP_TW + (CP_UW - 1 - ui);
            ok = true;
        } else {
            const int zt = wl >> 1, rowt = CP_TROWS - COS_P + (wl & 1);
            o = (wave * COS_P + zt) * PSZ + rowt * CP_TW + (CP_UW - 1 - ui);
            ok = zt < COS_P && (KY + 14 >= CP_TROWS - 1 || rowt < CP_TROWS - 1);
        }
    };
    auto ru_eval_all = [&](const int sa_f, const int sbb_f, unsigned (&hi_words)[CP_AHEAD_N], unsigned (&lo_words)[CP_AHEAD_N]) __attribute__((always_inline)) {
        int lane_o = lane;
        asm volatile("" : "+v"(lane_o));
        const int wl = lane_o >> 3, ui = lane_o & 7;
        const float U = (float)(ibase + P.x_begin + P.ux0 + P.mx * (ui - 7) - 8 * P.mx * sa_f);
        const float dx = fmaf(U, P.hx_hi, fmaf(U, P.hx_lo, P.fx0));
        const float dx2 = dx * dx;
        const int Wsb = jbase + P.uy0 + P.my * (wl - ROW0) - 8 * P.my * sbb_f;
        float dz2[COS_P];
#pragma unroll
        for (int z = 0; z < COS_P; ++z) dz2[z] = plane_dz2(z);
#pragma unroll
        for (int r = 0; r < RU_NR; ++r) {
            const float W = (float)(Wsb + RU_ROWS * P.my * r);
            const float dy = fmaf(W, P.hy_hi, fmaf(W, P.hy_lo, P.fy0));
            const float r2 = fmaf(dy, dy, dx2);
#pragma unroll
            for (int z = 0; z < COS_P; ++z) entry(r2, dz2[z], dx, dy, hi_words[COS_P * r + z], lo_words[COS_P * r + z]);
        }
        const int zt = wl >> 1, rowt = CP_TROWS - COS_P + (wl & 1);
        const float W = (float)(Wsb - P.my * wl + rowt * P.my);
        const float dy = fmaf(W, P.hy_hi, fmaf(W, P.hy_lo, P.fy0));
        float dzl = dz2[0];
#pragma unroll
        for (int z = 1; z < COS_P; ++z) dzl = zt == z ? dz2[z] : dzl;
        entry(fmaf(dy, dy, dx2), dzl, dx, dy, hi_words[CP_AHEAD_N - 1], lo_words[CP_AHEAD_N - 1]);
    };
    constexpr int CHUNK_U4 = PAIR * 4 * NT * B_KS_U4, PRE = CHUNK_U4 / THREADS;
    static_assert(CHUNK_U4 % THREADS == 0, "chunk must split evenly over the block");
    constexpr int REC_U4 = 4 * NT * B_KS_U4;     // uint4 per super-block: 4 K-step records x NT column tiles
    uint4 pre[PRE];
    const uint4* const bsrc = bfrag + (size_t)tile * n_sb * REC_U4;
    // (the steering fragments do not depend on the item: all items of a launch tile read the same chunks)
    // A request is one chunk = the PAIR super-blocks of a table pair, THREADS x PRE uint4.  n_sb is even and the launch tile holds n_sb whole
    // super-blocks (the host refuses a plan where either fails: olx.hip), so a chunk lies inside the tile's records as a whole or not at all:
    // ONE wave-uniform test per request (the caller's: a scalar compare and branch), no per-lane bounds test, select or zero fill; a lane's
    // address is a scalar base per q (q x 8192 bytes is beyond a global_load immediate) + its 32-bit byte offset tid x 16 -- one vector
    // instruction per request.  Per-lane tests and 64-bit per-lane addresses were 33 vector instructions per request, 25 of them executed
    // even by the last pair that requests nothing.
    auto request = [&](const int sb_first, const int tid_r) __attribute__((always_inline)) {
        const unsigned lane_b = (unsigned)tid_r << 4;
#pragma unroll
        for (int q = 0; q < PRE; ++q) {
            // (opaque scalar base: left to itself the compiler adds the lane offset first and then q x 8192 to the 64-bit per-lane address)
            unsigned first_q = (unsigned)(sb_first * REC_U4 + q * THREADS);      // the chunk's entry of lane 0
            asm volatile("" : "+s"(first_q));
            // (a typed 16-byte load and four component assignments: a struct copy under the uniform branch stays a memcpy into a private array -- scratch)
            typedef unsigned uintx4_t __attribute__((ext_vector_type(4)));
            uintx4_t v = {0u, 0u, 0u, 0u};
            if (OLX_IN((long long)sb_first * REC_U4 + tid_r + q * THREADS, (long long)n_sb * REC_U4, 4))      // (debug library: the lane's entry inside the launch tile's own records)
                v = *reinterpret_cast<const uintx4_t*>(reinterpret_cast<const unsigned char*>(bsrc + first_q) + lane_b);
            pre[q].x = v.x; pre[q].y = v.y; pre[q].z = v.z; pre[q].w = v.w;
        }
    };
    request(0, tid);        // the first pair: always there (n_sb >= PAIR)
    OLX_CUTRACE(1, (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) | ((unsigned long long)ntile << 8));      // XCC_ID | the wave's tiles << 8
    OLX_STAMP(0);
#ifdef OLX_EXP_STAMPS   // developer build only (tools/stamps_cosetp.py splits the phases by it): the wave's tile count in the low 3 bits of stamp 0
    if (lane == 0 && wave < 4 && blockIdx.y == 0 && blockIdx.x % 37 == 0 && blockIdx.x / 37 < 1024) {
        unsigned long long& s0 = g_stamps[(blockIdx.x / 37) * 4 + wave][0];
        s0 = (s0 & ~7ull) | (unsigned long long)ntile;
    }
#endif
    for (int sb0 = 0; sb0 < n_sb; sb0 += PAIR) {
        const int sa = sb0 / nsbp, sbb0 = sb0 - sa * nsbp;       // the pair (sa, sbb0), (sa, sbb0 + 1)
        // previous pair consumed: steering stage and tables are free.  (Not before the first pair: nothing to protect yet, and
        // __syncthreads() drains vmcnt -- the wave would wait for its first steering loads before the tables instead of behind them.)
        if (sb0 > 0) __syncthreads();
        // a pair whose predecessor in this block was (sa - 1, same sbb0) shares 4 of its 12 table columns with it: nsbp == PAIR (one pair per sa)
        const bool reuse = sb0 > 0 && reuse_ok;      // (block-uniform)
        if (sb0 == 0) OLX_STAMP(1);
        if (sb0 == 2) OLX_STAMP(7);
        // ---- G tables of planes 2 wave, 2 wave + 1: 26 rows x 12 offsets, shared by the pair's two super-blocks
        // (fp8 shape: table generation at raised priority -- the waves a block's K-steps wait for get the VALU first: -2 ... -4 %;
        // with fp16 corrections the matrix pipe is the scarcer resource and the same setting costs 1.5 %, priority on the K-steps 2.5 %)
        if constexpr (FP8) __builtin_amdgcn_s_setprio(1);
        const bool held = reuse && ahead_ok;          // (block-uniform) this pair's new columns were evaluated in front of the K-steps of the pair before it
        if (my_planes) {
            int lane_o = lane;
            asm volatile("" : "+v"(lane_o));
            float dz2[COS_P];
#pragma unroll
            for (int z = 0; z < COS_P; ++z) dz2[z] = plane_dz2(z);
            auto entry_put = [&](const float r2, const float dz2v, const float dx, const float dy, const int o, const bool ok) __attribute__((always_inline)) {
                unsigned hw, lw;
                entry(r2, dz2v, dx, dy, hw, lw);
                put(o, ok, hw, lw);
            };
            // The fill proper.  FULL form (reuse_c = 0): 12 columns x 5 rows per round -- rows 0 .. TROWS - 2 in whole rounds x the wave's
            // two planes, the LAST row once for both planes (row group wl takes plane wl): 11 instead of 12 evaluations per lane and pair.
            // REUSE form (reuse_c = 1, after the move below): only the 8 new columns ui = 0 .. 7, 8 columns x 8 rows per round -- rows 0 .. 23 in
            // 3 rounds x two planes, rows 24 and 25 of both planes in one more evaluation (lanes 0 .. 31): 7 evaluations per lane and pair.
            auto fill = [&](auto reuse_c) __attribute__((always_inline)) {
                constexpr bool RU = decltype(reuse_c)::value != 0;
                constexpr int CW = RU ? CP_UW - CP_SHARED : CP_UW;                  // columns evaluated
                constexpr int RPF = 64 / CW;                                        // table rows per round
                constexpr int NRF = (TROWS - (RU ? COS_P : 1)) / RPF;               // whole rounds
                static_assert(NRF * RPF == TROWS - (RU ? COS_P : 1) && (RU ? COS_P * COS_P : COS_P) <= RPF, "the tail rows fit one evaluation of the wave's planes");
                const int wl = lane_o / CW, ui = lane_o - CW * wl;
                const bool gen_lane = wl < RPF;
                const int Ulane = ibase + P.x_begin + P.ux0 + P.mx * (ui - 7);
                const int Wlane = jbase + P.uy0 + P.my * (wl - ROW0);
                const int tw_off = (wave * COS_P) * PSZ + wl * CP_TW + (CP_UW - 1 - ui);   // + z PSZ + RPF r TW
                const float U = (float)(Ulane - 8 * P.mx * sa);
                const float dx = fmaf(U, P.hx_hi, fmaf(U, P.hx_lo, P.fx0));
                const float dx2 = dx * dx;
                const int Wsb = Wlane - 8 * P.my * sbb0;
#pragma unroll 2
                for (int r = 0; r < NRF; ++r) {
                    const float W = (float)(Wsb + RPF * P.my * r);
                    const float dy = fmaf(W, P.hy_hi, fmaf(W, P.hy_lo, P.fy0));
                    const float r2 = fmaf(dy, dy, dx2);
#pragma unroll
                    for (int z = 0; z < COS_P; ++z) entry_put(r2, dz2[z], dx, dy, z * PSZ + tw_off + RPF * r * CP_TW, gen_lane);
                }
                // (block-uniform: the fragments of KY positions reach table rows 0 .. KY + 14)
                const bool last_row = KY + 14 >= TROWS - 1;
                if constexpr (RU) {          // row group wl: plane wl / 2, row TROWS - 2 + wl % 2
                    const int zt = wl >> 1, rowt = TROWS - COS_P + (wl & 1);
                    const float W = (float)(Wsb - P.my * wl + rowt * P.my);
                    const float dy = fmaf(W, P.hy_hi, fmaf(W, P.hy_lo, P.fy0));
                    float dzl = dz2[0];
#pragma unroll
                    for (int z = 1; z < COS_P; ++z) dzl = zt == z ? dz2[z] : dzl;
                    entry_put(fmaf(dy, dy, dx2), dzl, dx, dy, (wave * COS_P + zt) * PSZ + rowt * CP_TW + (CP_UW - 1 - ui), zt < COS_P && (last_row || rowt < TROWS - 1));
                } else if (last_row) {
                    const float W = (float)(Wsb - P.my * wl + (TROWS - 1) * P.my);
                    const float dy = fmaf(W, P.hy_hi, fmaf(W, P.hy_lo, P.fy0));
                    float dzl = dz2[0];
#pragma unroll
                    for (int z = 1; z < COS_P; ++z) dzl = wl == z ? dz2[z] : dzl;
                    entry_put(fmaf(dy, dy, dx2), dzl, dx, dy, (wave * COS_P + wl) * PSZ + (TROWS - 1) * CP_TW + (CP_UW - 1 - ui), wl < COS_P);
                }
            };
            if (reuse) {
                // the previous pair (sa - 1, same sbb0) left columns ud = [-7, -4] of THIS pair in words 8 .. 11 of every row (same U, dx, row and
                // plane: same bits).  Move them to words 0 .. 3: one lane per (plane, row) of the wave's own planes, two 8-byte reads and writes per
                // array (rows are 8-byte aligned).  The wave's LDS operations complete in order: the reads stay ahead of the fill's stores to words 8 .. 11.
                static_assert(COS_P * TROWS <= 64 && CP_UW - CP_SHARED == 8 && CP_TW % 2 == 0 && PSZ % 2 == 0, "one lane per (plane, row); aligned 8-byte moves");
                const int zm = lane_o >= TROWS ? 1 : 0;
                const int mo = (wave * COS_P + zm) * PSZ + (lane_o - zm * TROWS) * CP_TW;
                if (lane_o < COS_P * TROWS && OLX_IN(mo, T_WORDS - (CP_UW - 1), 3)) {
                    unsigned long long mv[4];
                    __builtin_memcpy(&mv[0], __builtin_assume_aligned(s_hi + mo + 8, 8), 8);
                    __builtin_memcpy(&mv[1], __builtin_assume_aligned(s_hi + mo + 10, 8), 8);
                    __builtin_memcpy(&mv[2], __builtin_assume_aligned(s_lo + mo + 8, 8), 8);
                    __builtin_memcpy(&mv[3], __builtin_assume_aligned(s_lo + mo + 10, 8), 8);
                    __builtin_memcpy(__builtin_assume_aligned(s_hi + mo, 8), &mv[0], 8);
                    __builtin_memcpy(__builtin_assume_aligned(s_hi + mo + 2, 8), &mv[1], 8);
                    __builtin_memcpy(__builtin_assume_aligned(s_lo + mo, 8), &mv[2], 8);
                    __builtin_memcpy(__builtin_assume_aligned(s_lo + mo + 2, 8), &mv[3], 8);
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // (no instruction: pins the move ahead of the fill's stores in the compiler's order too)
                if (held) {             // the 8 new columns: evaluated ahead, 14 stores per lane
#pragma unroll
                    for (int e = 0; e < CP_AHEAD_N; ++e) {
                        int o;
                        bool ok;
                        ru_slot(e, lane_o, o, ok);
                        put(o, ok, held_hi[e], held_lo[e]);
                    }
                } else {
                    fill(IntC<1>{});
                }
            } else {
                fill(IntC<0>{});
            }
        }
        if constexpr (FP8) __builtin_amdgcn_s_setprio(0);
        // this pair's steering fragments (requested one pair ahead; the first ones arrive behind the table generation above)
#pragma unroll
        for (int q = 0; q < PRE; ++q) reinterpret_cast<uint4*>(smem)[tid + q * THREADS] = pre[q];
        if (sb0 == 0) OLX_STAMP(2);
        __syncthreads();
        if (sb0 == 0) OLX_STAMP(3);
        // next pair's fragments: in flight during the K-steps, drained by the next barrier.  Where the wave holds fill-ahead words on top of the
        // fp8 shape's fragments (PRE_LATE) the request waits until the K-steps are through: the 16 registers of pre[] are not live across them
        // (held words + pre[] + the K-steps' 93 registers do not fit 128; requested at the last K-step group they spilled 2 - 6 registers).
        auto request_next = [&]() __attribute__((always_inline)) {
            int tid_o = tid;
            // (opaque.  PRE_LATE: the request stays where it is written.  The others: the loop-invariant sum of base and lane offset would be hoisted, held
            // as a 64-bit per-lane address across the pairs, and every part's offset added to it with vector instructions.)
            asm volatile("" : "+v"(tid_o));
            if (sb0 + PAIR < n_sb) {                                            // (wave-uniform: the whole next chunk or nothing)
                request(sb0 + PAIR, tid_o);
            } else if constexpr (PRE_LATE) {
                // no next pair: nothing is issued.  pre[] still counts as assigned on this path (no instruction) -- it is dead from the stage
                // write above to here, and a path that left it alone would keep its 16 registers live across the K-steps.  The stage write at
                // the top of the loop is never reached with these values.
#pragma unroll
                for (int q = 0; q < PRE; ++q) asm volatile("" : "=v"(pre[q].x), "=v"(pre[q].y), "=v"(pre[q].z), "=v"(pre[q].w));
            }
        };
        if constexpr (!PRE_LATE) request_next();
        // fill-ahead: the next pair's reuse-form entries in ONE piece in front of the first tiles, at priority 0, behind a wave-uniform scalar branch.
        // A wave without tiles still owns two planes of the table and evaluates them; a wave whose planes lie beyond nz evaluates nothing.
        // (Spread over the four (sl, kb) groups, or placed behind a later group or behind the K-steps, the same evaluations made the launch slower:
        // DESIGN 5.6.)
        if constexpr (AHEAD) if (ahead_ok && my_planes && sb0 + PAIR < n_sb) {      // (reuse_ok: the next pair is (sa + 1, sbb0))
            ru_eval_all(sa + 1, sbb0, held_hi, held_lo);
        }
#pragma unroll                                          // (unrolled: the pair position becomes part of the immediate table offsets)
        for (int sl = 0; sl < PAIR; ++sl) {
            if (sbb0 + sl >= P.nsb) break;              // padding super-block of an odd count: zero weights, nothing to do
            if constexpr (FP8) {
#pragma unroll
                for (int kb = 0; kb < 2; ++kb) {         // K-step pairs (ka = 0, 1): two fp16 hi*hi products + ONE fp8 product
                    Half8Bits bh[2][NT];
                    intx8_t b8[NT];
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
                        for (int ka = 0; ka < 2; ++ka) {
                            bh[ka][nt].u = s_B(sl * 4 + 2 * kb + ka, nt, 0)[lane];
                            const uint4 q = s_B(sl * 4 + 2 * kb + ka, nt, 1)[lane];
                            b8[nt][4 * ka + 0] = (int)q.x; b8[nt][4 * ka + 1] = (int)q.y; b8[nt][4 * ka + 2] = (int)q.z; b8[nt][4 * ka + 3] = (int)q.w;
                        }
                    }
                    const int nt_g = tile_count();
#pragma unroll
                    for (int t = 0; t < MT; ++t) {
                        if (t >= nt_g) continue;             // wave-uniform
                        Half8Bits ah[2];
                        intx8_t a8;
                        const int ro = (int)(frag_b[t] >> 2);      // the word index (read by the debug library's check alone)
#pragma unroll
                        for (int ka = 0; ka < 2; ++ka) {
                            const int kso = 4 * ka - (4 * kb + 8 * sl) * CP_TW;   // the pair's second super-block reads 8 table rows lower
                            if (!OLX_IN(ro + kso, T_WORDS - 3, 1)) continue;
                            const unsigned long long* ph2 = frag_at(s_hi, t, kso);
                            const unsigned long long* pl2 = frag_at(s_lo, t, kso);
                            const unsigned long long h0 = __hip_atomic_load(ph2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                            const unsigned long long h1 = __hip_atomic_load(ph2 + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                            const unsigned long long l0 = __hip_atomic_load(pl2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                            const unsigned long long l1 = __hip_atomic_load(pl2 + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                            ah[ka].w[0] = (unsigned)h0; ah[ka].w[1] = (unsigned)(h0 >> 32); ah[ka].w[2] = (unsigned)h1; ah[ka].w[3] = (unsigned)(h1 >> 32);
                            a8[4 * ka + 0] = (int)(unsigned)l0; a8[4 * ka + 1] = (int)(unsigned)(l0 >> 32);
                            a8[4 * ka + 2] = (int)(unsigned)l1; a8[4 * ka + 3] = (int)(unsigned)(l1 >> 32);
                        }
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt) acc[t][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[0].h, bh[0][nt].h, acc[t][nt], 0, 0, 0);
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt) acc[t][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[1].h, bh[1][nt].h, acc[t][nt], 0, 0, 0);
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt)      // E8M0 scales undo the operand scaling: 2^(128 - 127) * COS_F8_LO * COS_F8_HI = 1
                            acc[t][nt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a8, b8[nt], acc[t][nt], 0, 0, 0, 128, 0, 127);
                    }
                }
            } else {
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {         // unrolled: the K-step's table offset becomes an immediate
                    const int ka = ks & 1, kb = ks >> 1;
                    Half8Bits bh[NT], bl[NT];
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        bh[nt].u = s_B(sl * 4 + ks, nt, 0)[lane];
                        bl[nt].u = s_B(sl * 4 + ks, nt, 1)[lane];
                    }
                    const int kso = 4 * ka - (4 * kb + 8 * sl) * CP_TW;
                    const int nt_g = tile_count();
#pragma unroll
                    for (int t = 0; t < MT; ++t) {
                        if (t >= nt_g) continue;             // wave-uniform
                        Half8Bits ah, al;
                        const int ro = (int)(frag_b[t] >> 2);
                        if (!OLX_IN(ro + kso, T_WORDS - 3, 1)) continue;
                        const unsigned long long* ph2 = frag_at(s_hi, t, kso);
                        const unsigned long long* pl2 = frag_at(s_lo, t, kso);
                        const unsigned long long h0 = __hip_atomic_load(ph2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                        const unsigned long long h1 = __hip_atomic_load(ph2 + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                        const unsigned long long l0 = __hip_atomic_load(pl2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                        const unsigned long long l1 = __hip_atomic_load(pl2 + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                        ah.w[0] = (unsigned)h0; ah.w[1] = (unsigned)(h0 >> 32); ah.w[2] = (unsigned)h1; ah.w[3] = (unsigned)(h1 >> 32);
                        al.w[0] = (unsigned)l0; al.w[1] = (unsigned)(l0 >> 32); al.w[2] = (unsigned)l1; al.w[3] = (unsigned)(l1 >> 32);
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt) acc[t][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah.h, bh[nt].h, acc[t][nt], 0, 0, 0);
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt) acc[t][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al.h, bh[nt].h, acc[t][nt], 0, 0, 0);
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt) acc[t][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah.h, bl[nt].h, acc[t][nt], 0, 0, 0);
                    }
                }
            }
        }
        if constexpr (PRE_LATE) request_next();
        if (sb0 == 0) OLX_STAMP(4);
    }
    OLX_STAMP(5);
    // ---- epilogue, straight from the accumulators.  The steering fragments carry Re of column c in column tile 0 and Im of the same column
    // in column tile 1 (mfma_pack_k, split_reim), so lane (g, c16) holds BOTH parts of column c16 for rows 4 g .. 4 g + 3 = planes
    // k0 + 4 g .. + 3 of the tile's position: |p| and intensity in place without a lane exchange, two 16-byte stores per store target.
    // (Rounds 2 - 4 kept (Re, Im) in adjacent matrix columns as kernels 2c / 2e do: a quad swap per square, selects between the |p| lane
    // and the intensity lane, every address formed once per lane pair -- 48 instead of 12 vector instructions per position, 5 instead
    // of 3.5 per store: 939 -> 734 vector instructions per wave.  That alone changed the launch time by nothing -- profiles/r05_store_path.txt.)
    //   A  |p| / intensity over the accumulators (two rows per packed fp32 instruction), then the lane transpose below;
    //   B  per store-target slot of the lane's column (outer) the 64-bit bases of its focus volumes and its mirror masks once, then
    //      per tile (inner) offset = o00 + (fx & DX) + (fy & DY) with the three terms wave-uniform (scalar ALU), shared by both stores.
    int lane_e = lane;                                   // (opaque: the epilogue's per-lane constants -- targets, bases -- are formed here,
    asm volatile("" : "+v"(lane_e));                     // not kept in registers across the K-steps)
    // The accumulators put the four plane quads of a column 16 lanes apart; the vector memory unit takes a 16-byte store four LANES at a
    // time, so from there every 64-byte run goes out as four separate 16-byte requests.  One lane transpose first (ds_bpermute: the LDS
    // crossbar, no vector-ALU work): lane 4 c + g takes over column c, planes 4 g .. 4 g + 3 -- four consecutive lanes now write 64
    // contiguous bytes: -7 % on the launch (profiles/r05_store_path.txt).
    const int c16 = lane_e >> 2;
    const int kz = k0 + 4 * (lane_e & 3);
    const int src_lane4 = (16 * (lane_e & 3) + (lane_e >> 2)) * 4;      // byte index of the lane that computed this lane's values
    const float s_p = P.out_scale, s_i = P.out_scale * P.out_scale * P.inten_scale;
    const bool want_p = PONLY || (P.flags & 1u) != 0, want_i = !PONLY && (P.flags & 2u) != 0;      // (uniform)
    constexpr int NOUT = PONLY ? 1 : NT;                 // |p| alone: no intensity values, half the lane exchange
    const int nt_e = tile_count();
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        if (t >= nt_e) continue;
        float o[NOUT][4];
#pragma unroll
        for (int r = 0; r < 4; r += 2) {
            const float2_t re = {acc[t][0][r], acc[t][0][r + 1]}, im = {acc[t][1][r], acc[t][1][r + 1]};
            const float2_t m = __builtin_elementwise_fma(re, re, im * im);
            o[0][r] = __builtin_amdgcn_sqrtf(m.x) * s_p;
            o[0][r + 1] = __builtin_amdgcn_sqrtf(m.y) * s_p;
            if constexpr (!PONLY) {
                const float2_t in = m * float2_t{s_i, s_i};
                o[1][r] = in.x;
                o[1][r + 1] = in.y;
            }
        }
#pragma unroll
        for (int nt = 0; nt < NOUT; ++nt) {
            floatx4_t v;
            v[0] = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src_lane4, __builtin_bit_cast(int, o[nt][0])));
            v[1] = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src_lane4, __builtin_bit_cast(int, o[nt][1])));
            v[2] = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src_lane4, __builtin_bit_cast(int, o[nt][2])));
            v[3] = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src_lane4, __builtin_bit_cast(int, o[nt][3])));
            acc[t][nt] = v;
        }
    }
    if (kz < P.nz) {
    // store targets of this lane's column: focus * 4 + mirror image, -1 = none
    const int4 tq = *reinterpret_cast<const int4*>(targets + ((size_t)tile * (MFMA_COLS * MFMA_MAX_NT) + c16) * 4);
    const int xm = P.nx - 1, ym = P.ny - 1;
    const int sxz = P.ny * P.nz;
    // (the ragged-nz variant is a separate copy of the loop: with both store forms in one body the compiler merges them and
    // splits every 16-byte store into a 12-byte and a 4-byte instruction)
    auto readout = [&](auto full_c) {
        constexpr bool FULL4 = decltype(full_c)::value != 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int code = q == 0 ? tq.x : q == 1 ? tq.y : q == 2 ? tq.z : tq.w;
            if (code < 0) continue;
            const unsigned m = (unsigned)code & 3u;
            const bool fx = (MX == 2) && (m & 1u), fy = (MY == 2) && ((MX == 2) ? (m >> 1) : (m & 1u));
            unsigned fxm = fx ? 0xFFFFFFFFu : 0u, fym = fy ? 0xFFFFFFFFu : 0u;
            asm volatile("" : "+v"(fxm), "+v"(fym));      // (opaque: kept as masks -- one v_and per term instead of a move and a select)
            const long long fb = (long long)(code >> 2) * P.vox + kz;
            float* const base_p = pmag + fb;
            float* const base_i = inten + fb;
            const int nt_q = tile_count();
#pragma unroll
            for (int t = 0; t < MT; ++t) {
                if (t >= nt_q) continue;
                const int pos = wave + COS_NW * t;
                const int kx = (pos * ky_magic) >> 16, ky = pos - kx * KY;
                const int i = ibase + 2 * P.mx * kx, j = jbase + P.my * ky;      // wave-uniform (scalar ALU)
                const unsigned o00 = (unsigned)(i * sxz + j * P.nz);
                const unsigned DX = (unsigned)((xm - 2 * i) * sxz), DY = (unsigned)((ym - 2 * j) * P.nz);
                const unsigned off = o00 + (fxm & DX) + (fym & DY);
                if (!OLX_IN(fb + off + (FULL4 ? 3 : 0), (long long)P.n_foci * P.vox, 2)) continue;
                if constexpr (FULL4) {
                    if (BOTH || PONLY || want_p) *reinterpret_cast<floatx4u_t*>(base_p + off) = floatx4u_t{acc[t][0][0], acc[t][0][1], acc[t][0][2], acc[t][0][3]};
                    if (!PONLY && (BOTH || want_i)) *reinterpret_cast<floatx4u_t*>(base_i + off) = floatx4u_t{acc[t][1][0], acc[t][1][1], acc[t][1][2], acc[t][1][3]};
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (kz + e < P.nz) {
                            if (BOTH || PONLY || want_p) base_p[off + e] = acc[t][0][e];
                            if (!PONLY && (BOTH || want_i)) base_i[off + e] = acc[t][1][e];
                        }
                }
            }
        }
    };
    if (k0 + COS_ZB <= P.nz) readout(IntC<1>{}); else readout(IntC<0>{});      // (block-uniform: only a LAST, partial plane block stores plane by plane)
    }
    OLX_STAMP(6);
#ifdef OLX_EXP_CUTRACE
    OLX_CUTRACE(3, __builtin_readcyclecounter());
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    OLX_CUTRACE(4, __builtin_readcyclecounter());
#endif
    }
}

}  // namespace olx

using namespace olx;
OLX_BOUNDS_READER(cosetp)

#ifdef OLX_EXP_CUTRACE
extern "C" int olx_exp_read_cutrace_cosetp(unsigned long long* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(olx::g_cutrace), sizeof(unsigned long long) * 16384 * 8 * 5);
}
#endif
#ifdef OLX_EXP_STAMPS
extern "C" int olx_exp_read_stamps_cosetp(unsigned long long* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(olx::g_stamps), sizeof(unsigned long long) * 4096 * 8);
}
#endif

template <int MX, int MY>
static void launch_cosetp(olx_ctx* c, const LatticePart& q, float* pm) {
    CosetParams Q = c->cp;
#ifdef OLX_DEBUG_BOUNDS   // self-test of the debug build: pretend the output arrays hold one focus less -- the last focus' stores must be reported (and skipped)
    if (getenv("OLX_DEBUG_BOUNDS_SELFTEST")) Q.n_foci -= 1;
#endif
    float* inten_exp = c->d_inten;
    const bool clamp = c->clamp || c->lat.clamp;
    dim3 grid(q.n_blocks, c->mp.n_tiles), blk(COS_NW * 64);
    const bool both = (Q.flags & 3u) == 3u, ponly = (Q.flags & 3u) == 1u;      // |p| alone (OLX_OUT_PMAG: what the product plans) has its own epilogue
#define OLX_CP(CL, F8, DR) do { if (both) hipLaunchKernelGGL((field_cosetp_k<MX, MY, CL, F8, DR, true, false>), grid, blk, 0, c->stream, q.bfrag, pm, inten_exp, c->d_targets, q.blocks, Q); \
                                else if (ponly) hipLaunchKernelGGL((field_cosetp_k<MX, MY, CL, F8, DR, false, true>), grid, blk, 0, c->stream, q.bfrag, pm, inten_exp, c->d_targets, q.blocks, Q); \
                                else hipLaunchKernelGGL((field_cosetp_k<MX, MY, CL, F8, DR, false, false>), grid, blk, 0, c->stream, q.bfrag, pm, inten_exp, c->d_targets, q.blocks, Q); } while (0)
    if (c->dir_lattice) {   // piston directivity / uniform absorption folded into the geometry tables (fp16 corrections only)
        if (clamp) OLX_CP(true, false, true); else OLX_CP(false, false, true);
    } else if (q.fp8) {
        if (clamp) OLX_CP(true, true, false); else OLX_CP(false, true, false);
    } else {
        if (clamp) OLX_CP(true, false, false); else OLX_CP(false, false, false);
    }
#undef OLX_CP
}

void olx_launch_cosetp(olx_ctx* c, const LatticePart& q, float* pm) {
    if (c->mx == 2 && c->my == 2) launch_cosetp<2, 2>(c, q, pm);
    else if (c->mx == 2) launch_cosetp<2, 1>(c, q, pm);
    else if (c->my == 2) launch_cosetp<1, 2>(c, q, pm);
    else launch_cosetp<1, 1>(c, q, pm);
}
