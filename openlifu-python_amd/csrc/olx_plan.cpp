// Pure host planning of the lattice kernels: see olx_plan.h.  No HIP in this file -- it is also compiled by plain g++ with
// -fsanitize=address,undefined into the CPU-side checker (tools/plan_check.cpp).
#include "olx_plan.h"

#include "k_toep.hip.h"     // ToepShape: constants only, no device code

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace olxplan {

using namespace olx;

void build_slot_map(Lattice& L, int nsbp) {
    L.nsbp = nsbp; L.n_pad = L.nsa * nsbp * 64;
    L.slot_elem.assign((size_t)L.nsa * nsbp * 64, -1);
    for (int sa = 0; sa < L.nsa; ++sa)
        for (int sbb = 0; sbb < L.nsb; ++sbb)
            for (int ks = 0; ks < 4; ++ks)
                for (int bb = 0; bb < 4; ++bb)
                    for (int aa = 0; aa < 4; ++aa) {
                        const int a = 8 * sa + 4 * (ks & 1) + aa, b = 8 * sbb + 4 * (ks >> 1) + bb;
                        if (a < L.ax && b < L.ay)
                            L.slot_elem[((size_t)(sa * nsbp + sbb) * 4 + ks) * 16 + 4 * bb + aa] = L.cell[(size_t)a * L.ay + b];
                    }
}

// Kernel 2d precondition: the elements fill a regular ax x ay lattice in one z plane and the pitch is a whole number
// of voxels along x and y.  Fills L (slot map in 8 x 8 super-blocks of four 4 x 4 K-steps, padded with
// virtual elements) and the clamp / minimum-distance bounds including the virtual lattice points.
void detect_lattice(Lattice& L, bool flat, int n, const double* pos, const double spacing[3], const double lo[3], const double hi[3], double dmin) {
    L = Lattice();
    if (!flat || n < 16 || n > 16384) return;
    const double* X = pos;
    const double* Y = X + n;
    const double tol = 1e-10;
    auto axis = [&](const double* v, std::vector<double>& u) {
        u.assign(v, v + n);
        std::sort(u.begin(), u.end());
        size_t m = 0;
        for (size_t q = 0; q < u.size(); ++q)
            if (m == 0 || u[q] - u[m - 1] > tol) u[m++] = u[q];
        u.resize(m);
    };
    std::vector<double> xs, ys;
    axis(X, xs); axis(Y, ys);
    const int ax = (int)xs.size(), ay = (int)ys.size();
    if (ax < 2 || ay < 2 || (long long)ax * ay != n) return;
    const double px = (xs.back() - xs.front()) / (ax - 1), py = (ys.back() - ys.front()) / (ay - 1);
    for (int a = 0; a < ax; ++a) if (std::fabs(xs[a] - (xs[0] + a * px)) > tol) return;
    for (int b = 0; b < ay; ++b) if (std::fabs(ys[b] - (ys[0] + b * py)) > tol) return;
    const double rx = px / spacing[0], ry = py / spacing[1];
    const int mx = (int)std::llround(rx), my = (int)std::llround(ry);
    if (mx < 1 || my < 1 || std::fabs(rx - mx) > 1e-9 * mx || std::fabs(ry - my) > 1e-9 * my) return;
    const int nsa = (ax + 7) / 8, nsb = (ay + 7) / 8;
    if ((long long)nsa * nsb * 64 > 2LL * n) return;          // padding would more than double the contraction
    std::vector<int> cell((size_t)ax * ay, -1);
    for (int e = 0; e < n; ++e) {
        const int a = (int)std::llround((X[e] - xs[0]) / px), b = (int)std::llround((Y[e] - ys[0]) / py);
        if (a < 0 || a >= ax || b < 0 || b >= ay || cell[(size_t)a * ay + b] >= 0) return;
        cell[(size_t)a * ay + b] = e;
    }
    L.ax = ax; L.ay = ay; L.nsa = nsa; L.nsb = nsb;
    L.cell.swap(cell);
    build_slot_map(L, nsb);
    const int nsbp = (nsb + 1) & ~1;               // the bounds below also cover the padding rows of kernel 2e's pair tables
    // distance bounds over every lattice point of the padded array (virtual ones included: their G must stay finite)
    const double ez = pos[2 * (size_t)n];
    double min_d2 = 1e300; bool clamp = false;
    const double guard = 2.0 * dmin;
    for (int a = 0; a < std::max(8 * nsa, 16 * ((ax + 15) / 16)); ++a)   // (kernel 2f walks the columns in super-blocks of 16)
        for (int b = 0; b < 8 * nsbp; ++b) {          // (kernel 2e's pair table also covers the padding rows)
            const double p[3] = {xs[0] + a * px, ys[0] + b * py, ez};
            double d2 = 0;
            for (int k = 0; k < 3; ++k) {
                const double d = p[k] < lo[k] ? lo[k] - p[k] : (p[k] > hi[k] ? p[k] - hi[k] : 0.0);
                d2 += d * d;
            }
            min_d2 = std::min(min_d2, d2);
            if (d2 < guard * guard) clamp = true;
        }
    L.mx = mx; L.my = my;
    L.x0 = xs[0]; L.y0 = ys[0]; L.px = px; L.py = py; L.min_d2 = min_d2; L.clamp = clamp;
    L.ok = true;
}

// Kernel 2e: MFMA row tiles (16 rows) one plane pair needs over all cosets and parts -- per (coset, part)
// ceil(COS_P KX KY / 16) -- for a computed region of wx x wy voxels at lattice pitch (mx, my) voxels.
long long coset_tiles16(int wx, int wy, int mx, int my, int nt) {
    const int kxw = cos_kxw(nt);
    const int nsx = ((wx + 2 * mx - 1) / (2 * mx) + kxw - 1) / kxw, nsy = ((wy + my - 1) / my + COS_KYW - 1) / COS_KYW;
    long long t16 = 0;
    for (int rx = 0; rx < 2 * mx; ++rx)
        for (int ry = 0; ry < my; ++ry) {
            const int kxa = rx < wx ? (wx - 1 - rx) / (2 * mx) + 1 : 0, kya = ry < wy ? (wy - 1 - ry) / my + 1 : 0;
            for (int sx = 0; sx < nsx; ++sx)
                for (int sy = 0; sy < nsy; ++sy) {
                    const int KX = (sx + 1) * kxa / nsx - sx * kxa / nsx, KY = (sy + 1) * kya / nsy - sy * kya / nsy;
                    t16 += (COS_P * KX * KY + 15) / 16;
                }
        }
    return t16;
}

std::vector<int> mirror_perms(int n, int n_img, bool fold_x, bool fold_y, const int* px, const int* py, int rows) {
    std::vector<int> perm((size_t)rows * n);
    for (int m = 0; m < rows; ++m)
        for (int e = 0; e < n; ++e) {
            int o = e;
            const bool fx = fold_x && (m & 1), fy = fold_y && (fold_x ? (m >> 1) : (m & 1));
            if (m < n_img && fx) o = px[o];
            if (m < n_img && fy) o = py[o];
            perm[(size_t)m * n + e] = o;
        }
    return perm;
}

bool same_vector(const Steering& S, int f1, int m1, int f2, int m2) {
    const int n = S.n;
    for (int e = 0; e < n; ++e) {
        const size_t a = (size_t)f1 * n + S.perm[(size_t)m1 * n + e], b = (size_t)f2 * n + S.perm[(size_t)m2 * n + e];
        double dph = (S.delays[a] - S.delays[b]) * S.freq;
        dph -= std::nearbyint(dph);
        const double wa = S.apod[a] * S.area[a % n], wb = S.apod[b] * S.area[b % n];
        if (std::fabs(wa - wb) > 1e-12 * std::max(std::fabs(wa), std::fabs(wb))) return false;
        if (wa != 0.0 && std::fabs(dph) > 1e-9) return false;
    }
    return true;
}

// A column may store to ANY focus volume, so the search for an equal vector runs over every tile packed so far: mirror-partner
// foci share their columns wherever they sit in the sweep (a Wheel in its natural order has them at opposite ends).
Tiles pack_columns(const Steering& S, int maxc) {
    Tiles tl(1);
    for (int f = 0; f < S.F; ++f)
        for (int m = 0; m < S.n_img; ++m) {
            Col* hit = nullptr;
            for (size_t t = 0; t < tl.size() && !hit; ++t)
                for (size_t q = 0; q < tl[t].size() && !hit; ++q)
                    if (tl[t][q].ntgt < 4 && same_vector(S, tl[t][q].f, tl[t][q].m, f, m)) hit = &tl[t][q];
            if (!hit) {
                if ((int)tl.back().size() >= maxc) tl.emplace_back();
                tl.back().push_back(Col{f, m, 0, {-1, -1, -1, -1}});
                hit = &tl.back().back();
            }
            hit->tgt[hit->ntgt++] = f * 4 + m;
        }
    return tl;
}

void balance_store_targets(Tiles& tiles, int max_cols) {
    for (auto& t : tiles)
        for (size_t o = 0; o < t.size() && (int)t.size() < max_cols; ++o)
            if (t[o].ntgt > 2) {
                Col extra{t[o].f, t[o].m, 0, {-1, -1, -1, -1}};
                while (t[o].ntgt > 2) { extra.tgt[extra.ntgt++] = t[o].tgt[--t[o].ntgt]; t[o].tgt[t[o].ntgt] = -1; }
                t.push_back(extra);
            }
}

void coset_partition(CosetParams& Q, int kxw, int zb, int kyw) {
    const int px = Q.xs * Q.mx;      // voxels between two positions of a coset along x
    const int kx_max = (Q.nx - Q.x_lo + px - 1) / px, ky_max = (Q.ny - Q.y_lo + Q.my - 1) / Q.my;
    Q.nsx = (kx_max + kxw - 1) / kxw; Q.nsy = (ky_max + kyw - 1) / kyw;
    Q.kblocks = (Q.nz + zb - 1) / zb;
}

// blockIdx.x -> (coset, part, plane block), in the kernels' former decode order (the two blocks that write the two 64-byte halves of the
// same 128-byte lines get ids 8 apart = same XCD under round-robin dispatch)
bool build_coset_blocks(const CosetParams& Q, int zb, unsigned grp, int max_pos,
                        std::vector<CosetBlock>& blk, std::string& msg, bool heavy_first) {
    const int px = Q.xs * Q.mx;
    const unsigned nblk = (unsigned)(px * Q.my * Q.nsx * Q.nsy * Q.kblocks);
    blk.assign(nblk, CosetBlock{});
    const int wx = Q.nx - Q.x_lo, wy = Q.ny - Q.y_lo;
    // heavy_first (kernel 2g): the position sets are issued in the order of falling position count (stable) instead of the coset order, so that a CU's two
    // resident blocks are of one size for most of the launch and its last round is made of the lightest blocks (headline: 33-, 30-, 22-, then 20-position
    // blocks; measured in DESIGN 5.5).  The plane blocks of a set stay in a row on one XCD as before.  set_order: slot in the issue order -> position set.
    std::vector<unsigned> set_order;
    if (heavy_first) {
        const unsigned nsets = (unsigned)(px * Q.my * Q.nsx * Q.nsy);
        std::vector<int> npos_of(nsets);
        for (unsigned u = 0; u < nsets; ++u) {
            unsigned b = u;
            const int sy_part = (int)(b % (unsigned)Q.nsy); b /= (unsigned)Q.nsy;
            const int sx_part = (int)(b % (unsigned)Q.nsx); b /= (unsigned)Q.nsx;
            const int ry = (int)(b % (unsigned)Q.my), rx = (int)(b / (unsigned)Q.my);
            const int kx_all = rx < wx ? (wx - 1 - rx) / px + 1 : 0, ky_all = ry < wy ? (wy - 1 - ry) / Q.my + 1 : 0;
            const int KX = (sx_part + 1) * kx_all / Q.nsx - sx_part * kx_all / Q.nsx, KY = (sy_part + 1) * ky_all / Q.nsy - sy_part * ky_all / Q.nsy;
            npos_of[u] = (KX > 0 && KY > 0) ? KX * KY : 0;
        }
        set_order.resize(nsets);
        for (unsigned u = 0; u < nsets; ++u) set_order[u] = u;
        std::stable_sort(set_order.begin(), set_order.end(), [&](unsigned a, unsigned c) { return npos_of[a] > npos_of[c]; });
    }
    for (unsigned id = 0; id < nblk; ++id) {
        unsigned b = id;
        int kblock, ry_lo = 0;
        unsigned gy = 1;      // y cosets that follow each other on an XCD (grp > kblocks: grp = kblocks * gy)
        if (grp > (unsigned)Q.kblocks && grp % (unsigned)Q.kblocks == 0 && (unsigned)Q.my % (grp / (unsigned)Q.kblocks) == 0 && nblk % (8 * grp) == 0) {
            gy = grp / (unsigned)Q.kblocks;
            const unsigned xcd = b % 8, sft = b / 8, inner = sft % grp;
            kblock = (int)(inner % (unsigned)Q.kblocks); ry_lo = (int)(inner / (unsigned)Q.kblocks);
            b = (sft / grp) * 8 + xcd;
        } else if (grp <= (unsigned)Q.kblocks && (Q.kblocks % grp) == 0 && nblk % (8 * grp) == 0) {
            const unsigned xcd = b % 8, sft = b / 8, kb_lo = sft % grp, u = (sft / grp) * 8 + xcd, part = (unsigned)Q.kblocks / grp;
            kblock = (int)(grp * (u % part) + kb_lo); b = u / part;
        } else { kblock = (int)(b % (unsigned)Q.kblocks); b /= (unsigned)Q.kblocks; }
        if (gy == 1 && !set_order.empty()) b = set_order[b];      // (y cosets grouped on an XCD keep their order: a slot there is a group of sets)
        const int sy_part = (int)(b % (unsigned)Q.nsy); b /= (unsigned)Q.nsy;
        const int sx_part = (int)(b % (unsigned)Q.nsx); b /= (unsigned)Q.nsx;
        const unsigned myh = (unsigned)Q.my / gy;
        const int ry = (int)(b % myh) * (int)gy + ry_lo, rx = (int)(b / myh);
        const int kx_all = rx < wx ? (wx - 1 - rx) / px + 1 : 0, ky_all = ry < wy ? (wy - 1 - ry) / Q.my + 1 : 0;
        const int kx0 = sx_part * kx_all / Q.nsx, KX = (sx_part + 1) * kx_all / Q.nsx - kx0;
        const int ky0 = sy_part * ky_all / Q.nsy, KY = (sy_part + 1) * ky_all / Q.nsy - ky0;
        CosetBlock& B = blk[id];
        B.ibase = Q.x_lo + rx + px * kx0; B.jbase = Q.y_lo + ry + Q.my * ky0; B.k0 = kblock * zb;
        B.npos = (KX > 0 && KY > 0) ? KX * KY : 0; B.KY = KY > 0 ? KY : 1; B.ky_magic = 65536 / B.KY + 1; B.KX = KX > 0 ? KX : 0; B.pad_ = 0;
        if (max_pos > 0 && B.npos > max_pos) { msg = "a block part holds more than " + std::to_string(max_pos) + " positions"; return false; }
    }
    return true;
}

std::vector<int> build_store_jobs(const Tiles& tiles, int max_nt, int cols_per_nt, int jobs_per_tile, bool want_p, bool want_i) {
    const int ntiles = (int)tiles.size();
    std::vector<int> jobs((size_t)ntiles * max_nt * (jobs_per_tile + 1), -1);
    for (int t = 0; t < ntiles; ++t)
        for (int nt = 0; nt < max_nt; ++nt) {
            int* jb = &jobs[((size_t)t * max_nt + nt) * (jobs_per_tile + 1)];
            int cnt = 0;
            for (int c16 = 0; c16 < 16; ++c16) {
                const bool wantp = (c16 & 1) ? want_i : want_p;
                const size_t o = (size_t)nt * cols_per_nt + (c16 >> 1);
                if (!wantp || o >= tiles[t].size()) continue;
                for (int q = 0; q < 4; ++q) {
                    const int code = tiles[t][o].tgt[q];
                    if (code >= 0) jb[cnt++] = c16 | ((code & 3) << 4) | ((code >> 2) << 6);
                }
            }
            int lg = 0;
            while ((1 << lg) < cnt) ++lg;
            jb[jobs_per_tile] = lg;
        }
    return jobs;
}

// Foci of an externally supplied steering table (olx_set_steering; the run_simulation seam hands over delays only).  For the
// reference's geometric delays (bf/delay_methods/direct.py:28-38) tau_e = max(tof) - tof_e, every element satisfies
// |x - r_e| = S - s_e with s_e = c tau_e and one unknown S per focus; subtracting element 0's equation leaves a LINEAR system in
// (x, y, S) for a flat array:  -2 (r_e - r_0) . x + 2 (s_e - s_0) S = (s_e^2 - s_0^2) - (|r_e|^2 - |r_0|^2);  z follows from
// element 0 on the grid's side of the array.  Accepted only if the point reproduces all delays to 1e-6 m (lambda / 3750 at
// 400 kHz) -- arbitrary delay patterns have no such point and are reported as unknown.
bool infer_foci(bool flat, int n, int F, const double* pos, const double* delays, double c, double grid_z_mid, std::vector<double>& foci) {
    if (!flat || n < 4 || !delays) return false;
    const double* X = pos; const double* Y = X + n; const double* Z = Y + n;
    foci.assign(3 * (size_t)F, 0.0);
    for (int f = 0; f < F; ++f) {
        const double* tau = delays + (size_t)f * n;
        double A[3][4] = {{0}};   // normal equations [A | b] for u = (x, y, S)
        const double s0 = c * tau[0], q0 = X[0] * X[0] + Y[0] * Y[0];
        for (int e = 1; e < n; ++e) {
            const double se = c * tau[e];
            const double row[3] = {-2.0 * (X[e] - X[0]), -2.0 * (Y[e] - Y[0]), 2.0 * (se - s0)};
            const double rhs = (se * se - s0 * s0) - (X[e] * X[e] + Y[e] * Y[e] - q0);
            for (int i = 0; i < 3; ++i) {
                for (int j = 0; j < 3; ++j) A[i][j] += row[i] * row[j];
                A[i][3] += row[i] * rhs;
            }
        }
        for (int i = 0; i < 3; ++i) {   // Gaussian elimination with partial pivoting
            int piv = i;
            for (int r = i + 1; r < 3; ++r) if (std::fabs(A[r][i]) > std::fabs(A[piv][i])) piv = r;
            if (!(std::fabs(A[piv][i]) > 1e-300)) return false;
            if (piv != i) for (int j = 0; j < 4; ++j) std::swap(A[i][j], A[piv][j]);
            for (int r = 0; r < 3; ++r) {
                if (r == i) continue;
                const double m = A[r][i] / A[i][i];
                for (int j = i; j < 4; ++j) A[r][j] -= m * A[i][j];
            }
        }
        const double x = A[0][3] / A[0][0], y = A[1][3] / A[1][1], S = A[2][3] / A[2][2];
        const double dz2 = (S - s0) * (S - s0) - (x - X[0]) * (x - X[0]) - (y - Y[0]) * (y - Y[0]);
        if (!(dz2 > 0) || !std::isfinite(dz2)) return false;
        const double side = grid_z_mid >= Z[0] ? 1.0 : -1.0;
        const double z = Z[0] + side * std::sqrt(dz2);
        for (int e = 0; e < n; ++e) {
            const double d = std::sqrt((x - X[e]) * (x - X[e]) + (y - Y[e]) * (y - Y[e]) + (z - Z[e]) * (z - Z[e]));
            if (!(std::fabs(d - (S - c * tau[e])) <= 1e-6)) return false;
        }
        foci[3 * (size_t)f] = x; foci[3 * (size_t)f + 1] = y; foci[3 * (size_t)f + 2] = z;
    }
    return true;
}

double nearfield_s2(int n, const double* pos, const double origin[3], const double spacing[3], const int begin[3], const int count[3], double dclamp) {
    if (n <= 0) return 0.0;
    const double* P[3] = {pos, pos + n, pos + 2 * (size_t)n};
    const double dc2 = dclamp * dclamp;
    // candidates: every element for n <= 1024, else every stride-th one and the element nearest to the array's centroid
    // (regular arrays: the sum peaks next to the innermost elements, which have the most neighbours)
    const int stride = n <= 1024 ? 1 : (n + 1023) / 1024;
    int centre = 0;
    {
        double m[3] = {0, 0, 0}, best = 1e300;
        for (int a = 0; a < 3; ++a) { for (int e = 0; e < n; ++e) m[a] += P[a][e]; m[a] /= n; }
        for (int e = 0; e < n; ++e) {
            double d2 = 0;
            for (int a = 0; a < 3; ++a) d2 += (P[a][e] - m[a]) * (P[a][e] - m[a]);
            if (d2 < best) { best = d2; centre = e; }
        }
    }
    std::vector<int> cand;
    for (int e = 0; e < n; e += stride) cand.push_back(e);
    cand.push_back(centre);
    double s2max = 0.0;
    for (const int e0 : cand) {
        double v[3];
        for (int a = 0; a < 3; ++a) {
            long long i = std::llround((P[a][e0] - origin[a]) / spacing[a]);
            i = std::max<long long>(begin[a], std::min<long long>(i, (long long)begin[a] + count[a] - 1));
            v[a] = origin[a] + (double)i * spacing[a];
        }
        double s2 = 0.0;
        for (int e = 0; e < n; ++e) {
            const double dx = v[0] - P[0][e], dy = v[1] - P[1][e], dz = v[2] - P[2][e];
            s2 += 1.0 / std::max(dx * dx + dy * dy + dz * dz, dc2);
        }
        s2max = std::max(s2max, s2);
    }
    return s2max;
}

int fp8_first_plane(int n, const double* pos, const double* area, const double* apod, int F, const double* foci, const double origin[3],
                    const double spacing[3], const int gn[3], int x_begin, int x_count, const Lattice& L, std::vector<double>& nf_s2) {
    bool ok = true;
    double need = 0;        // the largest  FP8_ERR_K wmax_f / (FP8_ERR_BOUND peak_f)  over the foci: sqrt(S2) must stay below 1 / need
    for (int f = 0; ok && f < F; ++f) {
        for (int a = 0; a < 3; ++a) {
            const int b0 = a == 0 ? x_begin : 0, cnt = a == 0 ? x_count : gn[a];
            const double lo = origin[a] + (b0 - 0.5) * spacing[a];
            const double hi = origin[a] + (b0 + cnt - 0.5) * spacing[a];
            if (!(foci[3 * (size_t)f + a] >= lo && foci[3 * (size_t)f + a] <= hi)) ok = false;
        }
        double sw1 = 0, sw2 = 0, wmx = 0, peak = 0;
        const double* fo = &foci[3 * (size_t)f];
        for (int e = 0; e < n; ++e) {
            const double w = std::fabs(apod[(size_t)f * n + e] * area[e]);
            sw1 += w; sw2 += w * w; wmx = std::max(wmx, w);
            const double ddx = fo[0] - pos[e], ddy = fo[1] - pos[(size_t)n + e], ddz = fo[2] - pos[2 * (size_t)n + e];
            peak += w / std::sqrt(std::max(ddx * ddx + ddy * ddy + ddz * ddz, 1e-30));
        }
        if (!(sw2 > 0 && sw1 * sw1 / sw2 >= 255.5) || !(peak > 0)) ok = false;
        else need = std::max(need, FP8_ERR_K * wmx / (FP8_ERR_BOUND * peak));
    }
    if (!ok) return -1;
    // Voxels ON a symmetry plane of the array see its elements in pairs at exactly the same distance -- the same table entry, the same
    // rounding error, and for a focus on that plane the same weight: the pair's errors add coherently instead of at random.  On the array's
    // axis (both planes: grids with an odd voxel count centred on the array, e.g. the reference's default SimSetup) the emulation finds the
    // largest normalised error 1.5 x that of a grid whose voxels straddle the planes (4.2e-5 against 2.7 - 3.0e-5; the device measured
    // 9.2e-6 of the peak where the plain rule promised 7.5e-6): the rule's constant is raised by a quarter per plane that carries voxels.
    {
        int planes = 0;
        for (int a = 0; a < 2; ++a) {
            const double ctr = (a == 0 ? L.x0 + 0.5 * (L.ax - 1) * L.px : L.y0 + 0.5 * (L.ay - 1) * L.py);
            const double idx = (ctr - origin[a]) / spacing[a];
            const int b0 = a == 0 ? x_begin : 0, cnt = a == 0 ? x_count : gn[a];
            if (std::fabs(idx - std::round(idx)) <= 1e-6 && idx >= b0 - 0.5 && idx <= b0 + cnt - 0.5) ++planes;
        }
        need *= 1.0 + 0.25 * planes;
    }
    // the near field: the error next to an element is relative to that element's own term (olx_plan.h, FP8_ERR_K): the bound on the worst
    // voxel of the planes that run the e4m3 products must stay below FP8_ERR_BOUND of every focus' coherent peak.  S2 per first plane block:
    // derived lazily, once per (element table, planned slab) -- the caller resets the cache with the plan
    const int nzb = (gn[2] + COS_ZB - 1) / COS_ZB;
    if ((int)nf_s2.size() != nzb) nf_s2.assign(nzb, -1.0);
    for (int q = 0; q < nzb; ++q) {
        if (nf_s2[q] < 0) {
            const int b0[3] = {x_begin, 0, q * COS_ZB}, cnt[3] = {x_count, gn[1], gn[2] - q * COS_ZB};
            nf_s2[q] = nearfield_s2(n, pos, origin, spacing, b0, cnt, 0.5 * std::min({spacing[0], spacing[1], spacing[2]}));
        }
        if (need * std::sqrt(nf_s2[q]) <= 1.0) return q * COS_ZB;
    }
    return -1;
}

// A split launch is two launches and two operand sets: on BASELINE's array it pays from ~8 M (voxel, focus) pairs above the cut
// (121 x 121 x 81 planes x 8 foci: -13 %; the same grid with one focus +27 %, 61 x 61 x 33 x 8: +60 %; profiles/r06_time_grid.txt)
// -- and only while the cut leaves at least three quarters of the planes above it (cut at plane 48 of 256: -3 ... -12 %; at plane 80: +-0;
// profiles/r06_time_grid.txt); otherwise the whole launch keeps three fp16 products
bool fp8_split_pays(int x_count, int ny, int nz, int F, int cut) {
    return !((double)x_count * ny * (nz - cut) * F < 8.0e6 || 4 * cut > nz);
}

ToepPlan toep_plan(int ax, int mx, int my, int xs, int wx, int wy, int nz, bool dir_lattice, int saw_pin, int nm_pin) {
    ToepPlan T{};
    // kernel 2f: 8 positions along x per row tile; arrays up to 17 elements wide take TWO row tiles per block (<= 16 positions: the tiles share
    // tables and Toeplitz weights, k_toep.hip M2; wider arrays need the table's 32 columns for one tile: (8 - 1) + 24 = 31)
    T.saw = std::min(ax, saw_pin ? saw_pin : 24);
    // (NM = 2 reads the second tile's fragments 8 columns on in the same 32-word rows: arrays up to 17 wide; wider arrays take THREE tiles on 48-word rows
    // -- ToepShape<3>, k_toep.hip.h: one block per CU -- where that does not add padded position slots: BASELINE configs[3])
    T.nm = T.saw + 15 <= 32 ? 2 : 1;
    T.kyw = COS_KYW;
    const int zb = COS_ZB;      // planes per block
    const int kxa_max = wx > 0 ? (wx - 1) / (xs * mx) + 1 : 0, kya_max = wy > 0 ? (wy - 1) / my + 1 : 0;
    auto parts = [](int k, int w) { return std::max(1, (k + w - 1) / w); };
    if (T.nm == 2) {      // the two-row-tile shape computes both tiles of every block: only where a part holds more than 8 positions along x
        if ((kxa_max + parts(kxa_max, 16) - 1) / parts(kxa_max, 16) <= 8) T.nm = 1;
    } else if (!dir_lattice) {
        // position slots the matrix pipe works through, per coset and plane block: x parts x 8 NM, y parts x the wave groups that hold a position
        auto slots = [&](int nm, int kyw_, int nky) {
            const int px_ = parts(kxa_max, 8 * nm), py_ = parts(kya_max, kyw_);
            const int ky_part = (kya_max + py_ - 1) / py_;
            return (long long)px_ * 8 * nm * py_ * ((ky_part + nky - 1) / nky) * nky;
        };
        // (one block per CU in that shape: only where the launch still has a block for every CU)
        const long long nblk3 = (long long)xs * mx * my * parts(kxa_max, 24) * parts(kya_max, ToepShape<3>::KYW) * ((nz + zb - 1) / zb);
        const bool want3 = nm_pin ? nm_pin == 3 : (kxa_max > 8 && nblk3 >= 256 && 20 * slots(3, ToepShape<3>::KYW, ToepShape<3>::NKY) <= 21 * slots(1, ToepShape<1>::KYW, ToepShape<1>::NKY));
        if (want3) { T.nm = 3; T.kyw = ToepShape<3>::KYW; }
    }
    // element super-blocks of kernel 2f along x: the whole row for arrays up to 24 wide, else columns of 24 and the rest -- the table then has
    // (KXW - 1) + 24 = 31 <= 32 columns = two K-steps, and a last column of <= 8 elements fills K-step 1 only (ks_mask)
    T.nsa = (ax + T.saw - 1) / T.saw;
    if (T.nsa > 16) return T;      // (ks_mask holds 2 bits per column)
    for (int sa = 0; sa < T.nsa; ++sa) {
        const int wdt = std::min(T.saw, ax - sa * T.saw);      // elements of this column
        // table columns with weights: ud' = xs kx - al + (saw - 1), al < wdt, kx < KXW  ->  [saw - wdt, saw - 1 + xs (KXW - 1)]
        const int lo_c = T.saw - wdt, hi_c = T.saw - 1 + xs * (8 - 1);      // (of ONE row tile: the second tile of M2 reads the same fragments)
        unsigned m = 0;
        if (lo_c <= 15) m |= 1u;
        if (hi_c >= 16) m |= 2u;
        T.ks_mask |= m << (2 * sa);
        T.ksteps_total += (int)(m & 1u) + (int)(m >> 1);
        T.e4_units += (T.nm == 3 && m == 2u) ? 1 : 2;      // (three row tiles: a column with K-step 1 only takes its element rows in pairs, k_toep.hip)
    }
    return T;
}

// ---- the kernel-2 variant decision ----
bool steering_symmetric(int n, int F, const double* delays, const double* apod, const double* area, double freq, const int* perm) {
    if (!delays || !apod) return false;
    for (int f = 0; f < F; ++f)
        for (int e = 0; e < n; ++e) {
            const size_t a = (size_t)f * n + e, b = (size_t)f * n + perm[e];
            if (std::fabs(delays[a] - delays[b]) * freq > 1e-9) return false;
            if (std::fabs(apod[a] * area[e] - apod[b] * area[perm[e]]) > 1e-12 * std::fabs(apod[a] * area[e])) return false;
        }
    return true;
}

// kernel 2d applies when the array is a lattice commensurate with the grid and the pitch-strided row tiles
// (4 rows x pitch) do not overhang the computed region by more than 2x per axis
static bool lattice_fits(const VariantIn& in) {
    auto tile_fill = [](int width, int m) { const int blk = 4 * m; return (double)width / (double)(((width + blk - 1) / blk) * blk); };
    return in.allow_shared && in.lat->ok && (in.force_kind == 0 || in.force_kind == 4) &&
           tile_fill(in.fp.nx - (in.mx == 2 ? in.fp.nx / 2 : 0), in.lat->mx) >= 0.5 &&
           tile_fill(in.fp.ny - (in.my == 2 ? in.fp.ny / 2 : 0), in.lat->my) >= 0.5;
}

bool variant_reads_foci(const VariantIn& in) {
    return !in.hetero && lattice_fits(in) && in.pins.fp8 >= 0 && !(in.flags & (FLAG_FP16_CORRECTION | FLAG_OUT_COMPLEX)) && !in.modifier();
}

// One pass of the decision over `in` as it stands (decide_variant runs a second one for the fallback to kernels 2a-d).
// Steering-dependent: dx/dy = distinct weight columns along folded axes (1 when every focus' delays and apodization are
// mirror-symmetric), nf = foci per tile so that dx*dy*nf <= 8 accumulator columns.
static VariantPlan decide_pass(const VariantIn& in, std::vector<double>& nf_s2, int& slot_rows) {
    VariantPlan p;
    const int n = in.n, F = in.F;
    const Pins& pins = in.pins;
    const bool modifier = in.modifier(), cplx = (in.flags & FLAG_OUT_COMPLEX) != 0;
    p.mx = in.mx; p.my = in.my; p.allow_shared = in.allow_shared; p.dir_lattice = in.dir_lattice;
    const char* const clamp_tag = in.clamp ? "clamp" : "noclamp";
    if (in.hetero) {  // kernel 2h: no folds; the ray integrals of a (voxel, element) pair are shared by up to 8 foci per launch tile
        p.mx = p.my = 1;
        while (p.nf * 2 <= F && p.nf < 8) p.nf *= 2;
        char hb[160];
        if (in.marched)
            snprintf(hb, sizeof hb, "field_hmarch_k<nf%d,%s%s> (%d non-trivial planes, marched ray sums, %d launches)", p.nf,
                     clamp_tag, in.march_one ? ",one-sum" : "", in.n_planes, 2 * in.n_planes + 1);
        else if (in.n_layers > 0)
            snprintf(hb, sizeof hb, "field_hetero_k<4,nf%d,%s,layers> (%d non-trivial planes in %d layers of <= %d)", p.nf,
                     clamp_tag, in.n_planes, in.n_layers, in.planes_per_layer);
        else
            snprintf(hb, sizeof hb, "field_hetero_k<4,nf%d,%s> (%d non-trivial planes)", p.nf, clamp_tag, in.n_planes);
        p.variant = hb;
        return p;
    }
    p.dx = (p.mx == 2 && !steering_symmetric(n, F, in.delays, in.apod, in.area, in.freq, in.px)) ? 2 : 1;
    p.dy = (p.my == 2 && !steering_symmetric(n, F, in.delays, in.apod, in.area, in.freq, in.py)) ? 2 : 1;
    const int nm = p.dx * p.dy;
    if (p.allow_shared) while (p.nf * 2 <= F && p.nf * 2 * nm <= 8) p.nf *= 2;
    char nmbuf[384];
    const bool lat_ok = lattice_fits(in);
    if (modifier && !(lat_ok && p.dir_lattice)) {   // no lattice path for this array / grid: the exact per-pair kernel 2a-d
        p.allow_shared = false; p.dir_lattice = false;
        p.mx = p.my = p.dx = p.dy = p.nf = 1;
    }
    p.use_mfma = p.allow_shared && in.force_kind != 2 && (in.force_kind == 3 || nm * p.nf >= 2 || lat_ok) && (!modifier || lat_ok);
    p.use_lattice = p.use_mfma && lat_ok;
    const char* const near_tag = in.clamp ? "clamp" : (in.near ? "near" : "noclamp");
    if (p.use_mfma) {
        // ---- kernel 2c column plan.  A column = one distinct steering vector W[sigma_m(e), f]; every
        // (focus, mirror image) whose vector equals it (on-axis foci: all their images; mirror-partner foci of a
        // Wheel: each other's images) is a store TARGET of that column, so it is accumulated once.  Foci are packed
        // greedily into launch tiles of at most 32 columns (NT = 4 MFMA column tiles share each geometry fragment).
        const Lattice& A = *in.lat;
        const FieldParams& P = in.fp;
        const double rev = in.freq / in.c, lambda = in.c / in.freq;
        const int n_img = p.mx * p.my;
        constexpr int MAXC = MFMA_COLS * MFMA_MAX_NT;
        p.perm = mirror_perms(n, n_img, p.mx == 2, p.my == 2, in.px, in.py, 4);
        Steering SV;
        SV.n = n; SV.F = F; SV.n_img = n_img; SV.perm = p.perm.data(); SV.delays = in.delays; SV.apod = in.apod; SV.area = in.area; SV.freq = in.freq;
        const int wx = P.nx - (p.mx == 2 ? P.nx / 2 : 0), wy = P.ny - (p.my == 2 ? P.ny / 2 : 0);      // the computed region
        auto coset_fill = [&](int nt) {
            const long long t16 = coset_tiles16(wx, wy, A.mx, A.my, nt);
            return t16 > 0 ? (double)COS_P * wx * wy / (16.0 * (double)t16) : 0.0;
        };
        // e4m3 correction products (kernels 2e / 2f / 2g, NT <= 2) are the default wherever their error bound is a bound on the planned volume
        // (include/olx.h, olx_field_plan): the foci are known (olx_bf_solve in the element frame, or external delays that infer_foci
        // recognises as geometric: the caller resolves them), every focus lies inside the planned SLAB and has N_eff = (sum w)^2 / sum w^2 >= 256;
        // the plan flag OLX_FIELD_FP16_CORRECTION opts out, and so does OLX_FP8_CORRECTION=0.  Decided here, before the columns are packed: it also
        // decides the tile width below.  The rule itself is fp8_first_plane (first plane of the e4m3 products: 0 = every plane, a multiple of 16 = the
        // plane blocks below keep three fp16 products, -1 = not eligible).
        int fp8_cut = (variant_reads_foci(in) && in.foci)
                          ? fp8_first_plane(n, in.pos, in.area, in.apod, F, in.foci, in.origin, in.spacing, in.gn, in.x_begin, in.x_count, A, nf_s2) : -1;
        // The pin FORCES the e4m3 products past the eligibility rule -- results may then miss the 1e-5 gate, so only developer builds set it
        if (pins.fp8 > 0) fp8_cut = (lat_ok && !modifier) ? 0 : -1;
        // (a split launch is two launches and two operand sets: where it does not pay, the whole launch keeps three fp16 products)
        if (fp8_cut > 0 && !fp8_split_pays(in.x_count, in.gn[1], in.gn[2], F, fp8_cut)) fp8_cut = -1;
        const bool fp8_want = fp8_cut >= 0;
        p.fp8_kcut = fp8_want ? fp8_cut : 0;
        // A column may store to ANY focus volume, so the search for an equal vector runs over every tile packed so far: mirror-partner
        // foci share their columns wherever they sit in the sweep (a Wheel in its natural order has them at opposite ends).
        Tiles& tiles = p.tiles;
        tiles = pack_columns(SV, MAXC);
        // A sweep that needs SEVERAL launch tiles anyway is cut into tiles of 16 columns instead of 32: kernel 2g (NT = 2) then takes every
        // tile -- 8 x 0.43 ms against 2e's 4 x 0.92 ms on the 64-focus sweep (127 columns).  One tile of 17 - 32 columns stays with 2e's
        // NT = 4 shape when the fp16 corrections run (0.82 against 2 x 0.45 ms) and is cut in two when the e4m3 corrections apply, which
        // the NT = 4 shape has no registers for (2 x 0.39 against 0.86 ms).  OLX_FIELD_VARIANT=lattice keeps the 32-column tiles for A/B runs.
        {
            const bool wide = tiles.size() == 1 && (int)tiles[0].size() > MFMA_COLS * 2;
            if ((tiles.size() > 1 || (wide && fp8_want)) && p.use_lattice && !cplx && pins.family == FamilyPin::none && coset_fill(2) >= 0.6)
                tiles = pack_columns(SV, MFMA_COLS * 2);
        }
        for (auto& t : tiles) { p.total_cols += (int)t.size(); while (p.nt * MFMA_COLS < (int)t.size()) p.nt *= 2; }
        const int total_cols = p.total_cols;
        // kernel 2d saves table arithmetic but pays ~27 % padded MFMA rows on BASELINE's grids; with 4 column tiles per
        // geometry fragment the MFMAs dominate and kernel 2c's exact z-run tiling wins (measured, steady state, 64-focus
        // sweep: 4.6 vs 4.9 ms; 8-focus shard: 0.74 vs 0.58 ms) -- unless the family is pinned for A/B runs
        // Kernel 2e's NT = 4 shape (3 tiles per wave) takes the sweep when its tiles are reasonably full.
        if (p.use_lattice && p.nt >= 4 && in.force_kind != 4 && (cplx || coset_fill(p.nt) < 0.6)) p.use_lattice = false;
        // kernel 2e: whole cosets per wave (no row-tile padding, one table per plane); 2d stays for complex output and A/B runs.
        // MFMA tiles of kernel 2e: per (coset, part, plane pair) ceil(2 KX KY / 16); with very coarse pitches the position
        // grids get so small that most of a tile is padding -- then 2d's fixed 2 x 4 x 2 tiles are the better shape
        if (p.use_lattice) {
            FamilyPin fv = pins.family;
            if (modifier && fv != FamilyPin::lattice && fv != FamilyPin::lattice2d) fv = FamilyPin::none;   // (the A/B forms carry no per-term factors)
            p.use_coset = !cplx && fv != FamilyPin::lattice2d;
            if (coset_fill(p.nt) > 0 && coset_fill(p.nt) < 0.6 && fv != FamilyPin::lattice) p.use_coset = false;
            slot_rows = (p.use_coset && p.nt <= 2) ? ((A.nsb + 1) & ~1) : A.nsb;
            // kernel 2f: ONE distinct steering vector in the whole launch (an on-axis SinglePoint focus on a mirror-symmetric
            // array): Toeplitz weights stationary, 16 planes per MFMA tile -- 2e would use 2 of 16 matrix columns
            p.use_toep = p.use_coset && tiles.size() == 1 && total_cols == 1 && fv != FamilyPin::lattice;
            // kernel 2g: the NT = 2 shape with the planes in the MFMA rows (stores straight from the accumulators, no staging):
            // 6 - 9 % faster than 2e on the headline shard; OLX_FIELD_VARIANT=lattice pins kernel 2e for A/B runs
            p.use_cosetp = p.use_coset && !p.use_toep && p.nt == 2 && fv != FamilyPin::lattice;
            if (p.use_cosetp)   // kernel 2g stores per column slot: a column with 3 - 4 store targets (an on-axis focus) makes every
                balance_store_targets(tiles, p.nt * MFMA_COLS);   // lane wait for its extra passes -- hand half of them to a free column slot (same weights, no extra MFMA)
        }
        p.n_pad = p.use_lattice ? A.nsa * slot_rows * 64 : (n + 15) / 16 * 16;
        const int ntiles = (int)tiles.size();
        // [column][f, m] then [column][4 store targets]: one table, the store targets are its second part
        const size_t n_col = (size_t)ntiles * MAXC;
        p.colinfo.assign(n_col * 6, -1);
        for (int t = 0; t < ntiles; ++t)
            for (size_t o = 0; o < tiles[t].size(); ++o) {
                p.colinfo[((size_t)t * MAXC + o) * 2] = tiles[t][o].f;
                p.colinfo[((size_t)t * MAXC + o) * 2 + 1] = tiles[t][o].m;
                for (int q = 0; q < 4; ++q) p.colinfo[n_col * 2 + ((size_t)t * MAXC + o) * 4 + q] = tiles[t][o].tgt[q];
            }
        const double dmin_m = 0.5 * std::min({in.spacing[0], in.spacing[1], in.spacing[2]});
        p.lat_clamp = p.use_lattice && (in.clamp || A.clamp);
        const char* const lat_tag = p.lat_clamp ? "clamp" : "noclamp";
        const double min_dist = !p.use_lattice ? in.min_dist : (p.lat_clamp ? dmin_m : std::sqrt(A.min_d2));
        // power-of-two operand scales: |G| <= 1/d'_min, |W| <= wmax  ->  hi parts <= 2^14, lo parts normal
        const double dmin_w = std::max(min_dist * rev, 1e-6);
        const double sg = std::exp2(std::floor(std::log2(16384.0 * dmin_w)));
        double wmax = 0;
        for (size_t q = 0; q < (size_t)F * n; ++q) wmax = std::max(wmax, std::fabs(in.apod[q] * in.area[q % n]));
        wmax *= in.p0_pa / lambda * rev;
        const double sw = wmax > 0 ? std::exp2(std::floor(std::log2(16384.0 / wmax))) : 1.0;
        MfmaParams& M = p.mp;
        M.nx = P.nx; M.ny = P.ny; M.nz = P.nz; M.n_el_pad = p.n_pad; M.x_begin = P.x_begin; M.n_tiles = ntiles;
        M.hx = P.hx; M.hy = P.hy; M.hz = P.hz; M.dmin2 = P.dmin2; M.flat_ez = P.flat_ez; M.flat_kz = P.flat_kz; M.flat_fz = P.flat_fz;
        M.g_scale = (float)sg; M.out_scale = (float)(1.0 / (sg * sw)); M.inten_scale = P.inten_scale;
        M.vox = P.vox; M.flags = P.flags;
        p.g_scale = sg; p.out_scale = 1.0 / (sg * sw);
        p.mfma_wscale = in.p0_pa / lambda * rev * sw;
        if (p.use_lattice) {
            LatParams& L = p.lp;
            L.nx = P.nx; L.ny = P.ny; L.nz = P.nz;
            L.x_lo = p.mx == 2 ? P.nx / 2 : 0; L.y_lo = p.my == 2 ? P.ny / 2 : 0; L.x_begin = P.x_begin;
            L.mx = A.mx; L.my = A.my;
            L.tiles_x = ((P.nx - L.x_lo + 4 * A.mx - 1) / (4 * A.mx)) * 2 * A.mx;   // 2 x rows two pitches apart per tile
            L.tiles_y = ((P.ny - L.y_lo + 4 * A.my - 1) / (4 * A.my)) * A.my;       // 4 y rows one pitch apart
            L.kgroups = (P.nz + 2 * p.lat_mt - 1) / (2 * p.lat_mt);                 // lat_mt MFMA tiles per wave (2 planes each)
            L.nsa = A.nsa; L.nsb = A.nsb; L.nsbp = slot_rows;
            // dx(i, a) = (origin - x0) + (i - mx a) h: whole voxels go into the integer part, the rest is |f| <= h/2
            const double offx = in.origin[0] - A.x0, offy = in.origin[1] - A.y0;
            L.ux0 = (int)std::llround(offx / in.spacing[0]); L.uy0 = (int)std::llround(offy / in.spacing[1]);
            L.fx0 = (float)((offx - L.ux0 * in.spacing[0]) * rev); L.fy0 = (float)((offy - L.uy0 * in.spacing[1]) * rev);
            const double hxw = in.spacing[0] * rev, hyw = in.spacing[1] * rev;
            L.hx_hi = (float)hxw; L.hx_lo = (float)(hxw - (double)L.hx_hi);
            L.hy_hi = (float)hyw; L.hy_lo = (float)(hyw - (double)L.hy_hi);
            L.hz = P.hz; L.dmin2 = P.dmin2; L.flat_ez = P.flat_ez;
            L.g_scale = M.g_scale; L.out_scale = M.out_scale; L.inten_scale = P.inten_scale;
            L.vox = P.vox; L.flags = P.flags;
            const long long tiles16 = coset_tiles16(P.nx - L.x_lo, P.ny - L.y_lo, A.mx, A.my, p.nt);
            p.fp8corr = fp8_want && p.use_coset && cos_fp8(p.nt) && !modifier;      // (decided above, before the columns were packed)
            if (p.use_coset) {
                CosetParams& Q = p.cp;
                Q.nx = L.nx; Q.ny = L.ny; Q.nz = L.nz; Q.x_lo = L.x_lo; Q.y_lo = L.y_lo; Q.x_begin = L.x_begin; Q.mx = L.mx; Q.my = L.my;
                const int zb = COS_ZB;      // planes per block
                // positions of a coset along x: two pitches apart for kernels 2e / 2g (their fragment reads are 8-byte aligned that way), ONE for kernel 2f
                // (round 5: its 8-position row tiles then fill 7 - 8 of 8 slots on BASELINE's grids instead of 5 - 6, and its tables are shared by more rows)
                Q.xs = p.use_toep ? 1 : 2;
                // kernel 2f's block shape (one, two or three row tiles of 8 x positions, the element super-block columns and their K-steps): toep_plan
                ToepPlan& tp = p.toep;
                if (p.use_toep) tp = toep_plan(A.ax, Q.mx, Q.my, Q.xs, Q.nx - Q.x_lo, Q.ny - Q.y_lo, Q.nz, p.dir_lattice, pins.toep_saw, pins.toep_nm);
                const int kxw = p.use_toep ? 8 * tp.nm : cos_kxw(p.nt);
                coset_partition(Q, kxw, zb, tp.kyw);
                Q.nsa = L.nsa; Q.nsb = L.nsb; Q.nsbp = L.nsbp; Q.ux0 = L.ux0; Q.uy0 = L.uy0; Q.fx0 = L.fx0; Q.fy0 = L.fy0;
                Q.hx_hi = L.hx_hi; Q.hx_lo = L.hx_lo; Q.hy_hi = L.hy_hi; Q.hy_lo = L.hy_lo; Q.hz = L.hz;
                Q.dmin2 = L.dmin2; Q.flat_ez = L.flat_ez; Q.g_scale = L.g_scale; Q.out_scale = L.out_scale; Q.inten_scale = L.inten_scale;
                Q.vox = L.vox; Q.flags = L.flags; Q.n_foci = F;
#ifdef OLX_DEV_PINS
                Q.cp_noreuse = pins.cp_noreuse ? 1 : 0;             // (A/B) kernel 2g fills every table pair in full; the variant name says "noreuse"
                Q.cp_nofillahead = pins.cp_nofillahead ? 1 : 0;     // (A/B) kernel 2g keeps the reuse fill a phase of its own; the variant name says "nofillahead"
#endif
                p.heavy_first = p.use_cosetp && !pins.cp_nosort;    // kernel 2g's position sets heaviest first ((A/B) OLX_EXP_CP_NOSORT=1: the coset order; the variant name says "nosort")
                Q.dir_wx = (p.dir_lattice && in.directivity) ? (float)(0.5 * in.size0 / lambda) : 0.f;      // element width / length over 2 lambda (DIR instantiations)
                Q.dir_wy = (p.dir_lattice && in.directivity) ? (float)(0.5 * in.size1 / lambda) : 0.f;
                Q.absorb_l2 = p.dir_lattice ? (float)(in.absorb_np_m * lambda * 1.4426950408889634) : 0.f;   // exp(-a d) = exp2(-a lambda log2(e) d'), d' [wavelengths]
                // dense store-job lists per (launch tile, column tile): job = c16 | image << 4 | focus << 6
                p.jobs = build_store_jobs(tiles, MFMA_MAX_NT, MFMA_COLS, COS_JOBS, (P.flags & FLAG_OUT_PMAG) != 0, (P.flags & FLAG_OUT_INTENSITY) != 0);
                {   // kernel 2e / 2g / 2f block records: blockIdx.x -> (coset, part, plane block), in the kernels' former decode order.  The records
                    // themselves stay with the caller (build_coset_blocks, cached against rec_key: they depend on the partition only, not on the
                    // steering table -- 9 216 of them on the headline grid, 0.1 ms to derive and compare); decided here is their order over the XCDs.
                    // Plane blocks of one position set that follow each other on ONE XCD (round-robin dispatch: ids 8 apart): all 16 of them where the
                    // counts divide -- that XCD's L2 then collects whole 1 KB z lines of every voxel column before it writes them back.  Measured on the
                    // headline shard, alternating runs on one box: 1 / 2 / 4 / 8 / 16 in a row = 0.406 / 0.392 / 0.392 / 0.390 / 0.383 ms; y cosets
                    // grouped on top (48 - 192 in a row) 0.384 - 0.388 (profiles/r05_store_path.txt).  A/B: OLX_EXP_KGRP.
                    // (round 6: any count that divides the plane blocks, not only powers of two -- the reference's SimSetup grids have odd voxel counts,
                    // 257 planes = 17 plane blocks: without a group their 64-byte runs went to eight different L2s and the launch took 2.5 x as long)
                    auto pick_grp = [&](int kblocks) {
                        const unsigned long long nb = (unsigned long long)Q.xs * Q.mx * Q.my * Q.nsx * Q.nsy * kblocks;
                        for (int g2 = std::min(kblocks, 32); g2 >= 2; --g2) if (kblocks % g2 == 0 && nb % (8ull * g2) == 0) return (unsigned)g2;
                        return 1u;
                    };
                    const int kcut = p.fp8corr ? p.fp8_kcut : 0;      // records of the plane blocks from the cut on come FIRST (a launch of their own in the e4m3 arithmetic)
                    const int kb_near = kcut / zb, kb_far = Q.kblocks - kb_near;
                    p.kgrp = pick_grp(kb_far); p.kgrp_near = kb_near > 0 ? pick_grp(kb_near) : 0u;
                    if (pins.kgrp > 0) { p.kgrp = (unsigned)pins.kgrp; if (kb_near > 0) p.kgrp_near = p.kgrp; }
                    const int rec_key[17] = {Q.nx, Q.ny, Q.nz, Q.x_lo, Q.y_lo, Q.mx, Q.my, Q.nsx, Q.nsy, Q.kblocks, zb, (int)p.kgrp, p.use_cosetp ? 40 : 0, Q.xs, kcut, (int)p.kgrp_near,
                                             p.heavy_first ? 1 : 0};
                    memcpy(p.rec_key, rec_key, sizeof rec_key);
                    p.blocks_near = (unsigned)((unsigned long long)Q.xs * Q.mx * Q.my * Q.nsx * Q.nsy * kb_near);
                }
                // what the DENSE contraction of this launch needs, in the same units (one v_mfma_f32_16x16x32_f16 = 8192 real multiply-adds): computed
                // voxels x elements x columns x 4 real products per complex one, times the products of the operand split -- bench.py reports
                // dense / issued as `mfma_useful` (padding of rows, columns, K slots and the Toeplitz band all show up there)
                // (a launch split at fp8_kcut: the plane blocks below the cut run three fp16 products -- the matrix units of both parts are weighted by their planes)
                const double far_frac = p.fp8corr ? (double)std::max(0, P.nz - p.fp8_kcut) / (double)P.nz : 0.0;
                const double corr_units = 3.0 - far_frac;                                   // 2 with e4m3 corrections everywhere, 3 with fp16 x 3
                const std::string f8tag = !p.fp8corr ? "" : (p.fp8_kcut > 0 ? ",fp8corr from plane " + std::to_string(p.fp8_kcut) : ",fp8corr");
                p.n_dense = (long long)((double)(P.nx - L.x_lo) * (P.ny - L.y_lo) * P.nz * (double)n * total_cols * 4.0 / 8192.0 * corr_units);
                if (p.use_toep) {
                    // matrix-pipe units (one v_mfma_f32_16x16x32_f16 = 16 cycles): per block and element row, for each of its KY y positions 2 K-steps x 3 fp16
                    // products -- or, with e4m3 corrections, 2 fp16 products + one K = 128 e4m3 instruction (2 units)
                    // per element row and y position: 3 fp16 products per non-zero K-step, or 1 per non-zero K-step + one e4m3 instruction (2 units) per column
                    // (two row tiles, e4m3: rows in quads with paired K-step-1 operands -- 6 fp16 products + 3 e4m3 instructions per four rows: 3 units per row, k_toep.hip)
                    const double units_e4m3 = tp.nm == 2 ? 3.0 : (double)tp.ksteps_total + (double)tp.e4_units;
                    const double per_row = far_frac * units_e4m3 + (1.0 - far_frac) * 3.0 * tp.ksteps_total;
                    for (int rx = 0; rx < Q.xs * A.mx; ++rx)
                        for (int ry = 0; ry < A.my; ++ry) {
                            const int kxa = rx < wx ? (wx - 1 - rx) / (Q.xs * A.mx) + 1 : 0, kya = ry < wy ? (wy - 1 - ry) / A.my + 1 : 0;
                            for (int sx = 0; sx < Q.nsx; ++sx)
                                for (int sy = 0; sy < Q.nsy; ++sy) {
                                    const int KX = (sx + 1) * kxa / Q.nsx - sx * kxa / Q.nsx, KY = (sy + 1) * kya / Q.nsy - sy * kya / Q.nsy;
                                    if (KX > 0 && KY > 0) p.n_mfma += (long long)((double)KY * per_row * (tp.nm > 1 ? 8 * tp.nm : 8) * A.nsb * Q.kblocks);      // (row tiles of 8 positions: every tile of the block's shape is computed)
                                }
                        }
                    snprintf(nmbuf, sizeof nmbuf, "field_toep%s_k<mx%d,my%d,flat,%s%s> %d columns for %d foci x %d images in %d tile(s); "
                             "%dx%d lattice, pitch %dx%d voxels, %lld MFMA/launch (%lld dense), %d row tile(s) x %d y positions per block", "", p.mx, p.my, lat_tag, f8tag.c_str(),
                             total_cols, F, n_img, ntiles, A.ax, A.ay, A.mx, A.my, p.n_mfma, p.n_dense, tp.nm, tp.kyw);
                } else {
                    // matrix-pipe time in units of one v_mfma_f32_16x16x32_f16 (16 cycles): 3 fp16 products per K-step, or with fp8
                    // corrections 1 fp16 product per K-step + one K = 128 e4m3 instruction (2 units) per two K-steps
                    p.n_mfma = (long long)((double)tiles16 * ((P.nz + COS_P - 1) / COS_P) * A.nsa * A.nsb * 4 * p.nt * corr_units * ntiles);
                    if (p.use_cosetp) {   // kernel 2g: one row tile per position and 16-plane block, no padded rows
                        long long npos_all = 0;
                        for (int rx = 0; rx < 2 * A.mx; ++rx)
                            for (int ry = 0; ry < A.my; ++ry)
                                npos_all += (long long)(rx < wx ? (wx - 1 - rx) / (2 * A.mx) + 1 : 0) * (ry < wy ? (wy - 1 - ry) / A.my + 1 : 0);
                        p.n_mfma = (long long)((double)npos_all * Q.kblocks * A.nsa * A.nsb * 4 * p.nt * corr_units * ntiles);
                    }
#ifdef OLX_DEV_PINS
                    const std::string pin_tags = std::string((p.use_cosetp && pins.cp_noreuse) ? ",noreuse" : "") + ((p.use_cosetp && pins.cp_nofillahead) ? ",nofillahead" : "") +
                                                 ((p.use_cosetp && pins.cp_nosort) ? ",nosort" : "");
#else
                    const std::string pin_tags;      // (the product cannot name the tags: tests/test_gpu_cosetp_fill_ahead.py)
#endif
                    snprintf(nmbuf, sizeof nmbuf, "field_coset%s_k<nt%d,mx%d,my%d,flat,%s%s%s> %d columns for %d foci x %d images in %d tile(s); "
                             "%dx%d lattice, pitch %dx%d voxels, %lld MFMA/launch (%lld dense)", p.use_cosetp ? "p" : "", p.nt, p.mx, p.my, lat_tag,
                             f8tag.c_str(), pin_tags.c_str(), total_cols, F, n_img, ntiles, A.ax, A.ay, A.mx, A.my, p.n_mfma, p.n_dense);
                }
            } else {
                p.n_mfma = (long long)L.tiles_x * L.tiles_y * L.kgroups * A.nsa * A.nsb * 4 * p.lat_mt * p.nt * 3 * ntiles;
                snprintf(nmbuf, sizeof nmbuf, "field_lattice_k<mt%d,nt%d,mx%d,my%d,flat,%s> %d columns for %d foci x %d images in %d tile(s); "
                         "%dx%d lattice, pitch %dx%d voxels, %lld MFMA/launch", p.lat_mt, p.nt, p.mx, p.my, lat_tag,
                         total_cols, F, n_img, ntiles, A.ax, A.ay, A.mx, A.my, p.n_mfma);
            }
        } else {
            snprintf(nmbuf, sizeof nmbuf, "field_mfma_k<mt%d,nt%d,mx%d,my%d,%s,%s> %d columns for %d foci x %d images in %d tile(s)",
                     P.nz >= 48 ? 4 : 1, p.nt, p.mx, p.my, in.flat ? "flat" : "general", near_tag, total_cols, F, n_img, ntiles);
        }
    } else if (p.mx * p.my * p.nf == 1) {
        if (modifier) snprintf(nmbuf, sizeof nmbuf, "field_accum_dir_k<4,%s> (%s%s%s)", clamp_tag, in.directivity ? "piston directivity" : "",
                               (in.directivity && in.absorb_np_m > 0) ? ", " : "", in.absorb_np_m > 0 ? "uniform absorption" : "");
        else snprintf(nmbuf, sizeof nmbuf, "field_accum_k<4,%s,%s>", in.flat ? "flat" : "general", near_tag);
    } else {
        p.perm = mirror_perms(n, nm, p.dx == 2, p.dy == 2, in.px, in.py, nm);
        snprintf(nmbuf, sizeof nmbuf, "field_shared_k<4,mx%d,my%d,dx%d,dy%d,nf%d,%s,%s>", p.mx, p.my, p.dx, p.dy, p.nf, in.flat ? "flat" : "general", near_tag);
    }
    if (in.directivity && p.use_mfma) strncat(nmbuf, " +piston directivity in the tables", sizeof nmbuf - strlen(nmbuf) - 1);
    if (in.absorb_np_m > 0 && p.use_mfma) strncat(nmbuf, " +uniform absorption in the tables", sizeof nmbuf - strlen(nmbuf) - 1);
    p.variant = nmbuf;
    return p;
}

VariantPlan decide_variant(const VariantIn& in, std::vector<double>& nf_s2, int& slot_rows) {
    VariantPlan p = decide_pass(in, nf_s2, slot_rows);
    if (in.modifier() && p.use_mfma && !(p.use_lattice && p.use_coset)) {   // only the coset kernels (2e / 2f / 2g) carry per-term factors: fall back to 2a-d
        VariantIn exact = in;
        exact.mx = p.mx; exact.my = p.my; exact.dir_lattice = false; exact.allow_shared = false;
        p = decide_pass(exact, nf_s2, slot_rows);
    }
    return p;
}

bool build_variant_blocks(const VariantPlan& p, std::vector<CosetBlock>& blk, std::string& msg) {
    const int zb = COS_ZB, kcut = p.fp8corr ? p.fp8_kcut : 0, kb_near = kcut / zb, max_pos = p.use_cosetp ? 40 : 0;
    // each side of the cut gets its own record list (plane blocks of a position set in a row per XCD within the side)
    CosetParams Qf = p.cp; Qf.kblocks = p.cp.kblocks - kb_near;
    if (!build_coset_blocks(Qf, zb, p.kgrp, max_pos, blk, msg, p.heavy_first)) return false;
    for (CosetBlock& b : blk) b.k0 += kcut;
    if (kb_near > 0) {
        std::vector<CosetBlock> near;
        CosetParams Qn = p.cp; Qn.kblocks = kb_near;
        if (!build_coset_blocks(Qn, zb, p.kgrp_near, max_pos, near, msg, p.heavy_first)) return false;
        blk.insert(blk.end(), near.begin(), near.end());
    }
    return true;
}

}  // namespace olxplan

