// CPU-side checker of the lattice kernels' host planning (openlifu-python_amd/csrc/olx_plan.cpp), built by tests/test_plan_host.py with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/plan_check.cpp openlifu-python_amd/csrc/olx_plan.cpp
// and run over seeded fuzz shapes: arrays that pad to super-blocks, pitches of 1 .. 12 voxels, grids that cut cosets into unequal
// parts, ragged plane counts, folded / unfolded axes, x-slabs, 1 .. 64 foci with shared and distinct steering vectors.  Invariants:
//   lattice      every element sits in exactly one K slot, virtual slots are -1, the slot map has nsa x nsbp x 64 entries
//   columns      every (focus, image) is a store target of exactly one column, all targets of a column carry the same steering vector,
//                tiles hold at most maxc columns, at most 4 (2 after balancing, where slots were free) targets per column
//   blocks       the positions of all records x their plane blocks cover every voxel of the computed region exactly once, lie inside it,
//                respect the per-part limit, and the kernels' magic division pos / KY is exact for every position; kernel 2g's order (the position
//                sets heaviest first) covers the same voxels, keeps the plane blocks of a set 8 ids apart, and its position counts never rise along an XCD
//   store jobs   the dense job lists name exactly the targets of their columns
//   foci         geometric delays are recognised and reproduce the foci; scrambled delays are refused
//   mirrors      every row of mirror_perms is a permutation and an involution, row 0 and the rows past the image count are the identity, the row of
//                both folds is the composition of the single folds
//   e4m3 rule    fp8_first_plane / fp8_split_pays: known decisions on BASELINE's array, one case per way the rule refuses, the result against a
//                restatement that asks nearfield_s2 of every plane block without the cache
//   kernel 2f    toep_plan: known shapes of the project; the columns cover the array, ks_mask has 1 - 2 bits per column and none beyond
//   decision     decide_variant on every recognised lattice with 1 / 3 / 8 / 9 / 64 foci, plain and complex output, once with a per-term factor: the
//                family flags imply each other, e4m3 products only in the NT <= 2 coset shapes, NT covers the widest tile, colinfo / store jobs /
//                permutations sized as the kernels index them, an even row count of the pair tables for NT <= 2, no per-term factor left with a
//                kernel that carries none, and the record key names every quantity of the block records (one key, one record list)
// Exit code 0 = all shapes passed; any violation prints the shape and exits 1 (sanitizer reports abort on their own).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "../openlifu-python_amd/csrc/olx_plan.h"
#include "../openlifu-python_amd/csrc/k_toep.hip.h"

using namespace olx;
using namespace olxplan;

static int g_fail = 0;
static long long g_lattices = 0, g_records = 0, g_columns = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_fail; fprintf(stderr, "FAIL %s:%d (%s): ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); if (g_fail > 20) exit(1); } } while (0)

// the checker's own notion of "the same steering vector" (independent of the planner's): equal drive weights and equal phases (mod one period)
static bool ref_same_vector(const Steering& S, int f1, int m1, int f2, int m2) {
    for (int e = 0; e < S.n; ++e) {
        const int e1 = S.perm[(size_t)m1 * S.n + e], e2 = S.perm[(size_t)m2 * S.n + e];
        const double w1 = S.apod[(size_t)f1 * S.n + e1] * S.area[e1], w2 = S.apod[(size_t)f2 * S.n + e2] * S.area[e2];
        if (std::fabs(w1 - w2) > 1e-9 * std::max(std::fabs(w1), std::fabs(w2))) return false;
        if (w1 == 0.0) continue;
        const double turns = (S.delays[(size_t)f1 * S.n + e1] - S.delays[(size_t)f2 * S.n + e2]) * S.freq;
        if (std::fabs(turns - std::round(turns)) > 1e-6) return false;
    }
    return true;
}

// mirror_perms: [rows][n]; hpx / hpy = the checker's own axis mirrors of the element set
static void check_mirror_perms(const std::vector<int>& perm, int n, int n_img, bool fold_x, bool fold_y, const std::vector<int>& hpx, const std::vector<int>& hpy, int rows) {
    CHECK((int)perm.size() == rows * n, "mirror_perms: %zu entries for %d rows of %d", perm.size(), rows, n);
    if ((int)perm.size() != rows * n) return;
    auto at = [&](int m, int e) { return perm[(size_t)m * n + e]; };
    for (int m = 0; m < rows; ++m) {
        std::vector<int> seen(n, 0);
        for (int e = 0; e < n; ++e) {
            const int o = at(m, e);
            CHECK(o >= 0 && o < n, "mirror_perms: row %d maps %d to %d", m, e, o);
            if (o < 0 || o >= n) return;
            seen[o]++;
        }
        for (int e = 0; e < n; ++e) {
            CHECK(seen[e] == 1, "mirror_perms: row %d is no permutation (element %d hit %d times)", m, e, seen[e]);
            CHECK(at(m, at(m, e)) == e, "mirror_perms: row %d is no involution at element %d", m, e);
            if (m == 0 || m >= n_img) CHECK(at(m, e) == e, "mirror_perms: row %d (images %d) is not the identity", m, n_img);
        }
    }
    // image bits: x fold = bit 0 where x is folded, y fold = the next bit
    const int bx = fold_x ? 1 : 0, by = fold_y ? (fold_x ? 2 : 1) : 0;
    for (int e = 0; e < n; ++e) {
        if (bx && bx < std::min(n_img, rows)) CHECK(at(bx, e) == hpx[e], "mirror_perms: the x fold's row is not the x mirror");
        if (by && by < std::min(n_img, rows)) CHECK(at(by, e) == hpy[e], "mirror_perms: the y fold's row is not the y mirror");
        if (bx && by && 3 < std::min(n_img, rows)) CHECK(at(3, e) == at(by, at(bx, e)), "mirror_perms: the row of both folds is not the composition of the single folds");
    }
}

struct Shape {
    int nax, nay, mxv, myv;        // elements per axis, pitch in voxels
    int n[3];                      // grid
    int x_begin, x_count;          // slab
    bool fold_x, fold_y;           // mirror folds (grid centred on the array)
    int nf;                        // foci
    double h;                      // spacing [m]
};

struct Geometry { int n; const double* pos; const double* area; const int* px; const int* py; double origin[3]; double h; int gn[3]; int x_begin, x_count, mx, my; const Lattice* L; };
static void check_decision(const Geometry& G, int F, bool cplx, bool absorb);

static void check_shape(const Shape& S, std::mt19937_64& rng, int nt_force) {
    const int n = S.nax * S.nay;
    // ---- the array: lattice points in (a, b) order shuffled (element order must not matter), z = 0
    std::vector<int> order(n);
    for (int e = 0; e < n; ++e) order[e] = e;
    std::shuffle(order.begin(), order.end(), rng);
    std::vector<double> pos(3 * (size_t)n), area(n, 1e-6);
    const double px = S.mxv * S.h, py = S.myv * S.h;
    for (int q = 0; q < n; ++q) {
        const int a = order[q] / S.nay, b = order[q] % S.nay;
        pos[q] = (a - 0.5 * (S.nax - 1)) * px; pos[(size_t)n + q] = (b - 0.5 * (S.nay - 1)) * py; pos[2 * (size_t)n + q] = 0.0;
    }
    const double spacing[3] = {S.h, S.h, S.h};
    // grid: centred on the array where folded, shifted by a whole number of voxels plus a fraction otherwise
    double origin[3] = {-(S.n[0] - 1) * 0.5 * S.h + (S.fold_x ? 0.0 : 2.25 * S.h), -(S.n[1] - 1) * 0.5 * S.h + (S.fold_y ? 0.0 : -1.5 * S.h), 4e-3};
    double lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
        const int b0 = a == 0 ? S.x_begin : 0, cnt = a == 0 ? S.x_count : S.n[a];
        lo[a] = origin[a] + b0 * spacing[a]; hi[a] = origin[a] + (b0 + cnt - 1) * spacing[a];
    }
    Lattice L;
    detect_lattice(L, true, n, pos.data(), spacing, lo, hi, 0.5 * S.h);
    if ((long long)((S.nax + 7) / 8) * ((S.nay + 7) / 8) * 64 > 2LL * n) { CHECK(!L.ok, "padding rule"); return; }
    CHECK(L.ok && L.ax == S.nax && L.ay == S.nay && L.mx == S.mxv && L.my == S.myv, "lattice %dx%d pitch %dx%d not recognised", S.nax, S.nay, S.mxv, S.myv);
    if (!L.ok) return;
    ++g_lattices;
    for (int nsbp : {L.nsb, (L.nsb + 1) & ~1}) {
        build_slot_map(L, nsbp);
        CHECK((int)L.slot_elem.size() == L.nsa * nsbp * 64 && L.n_pad == L.nsa * nsbp * 64, "slot map size");
        std::vector<int> seen(n, 0);
        for (int v : L.slot_elem) { CHECK(v >= -1 && v < n, "slot value %d", v); if (v >= 0) seen[v]++; }
        for (int e = 0; e < n; ++e) CHECK(seen[e] == 1, "element %d in %d slots", e, seen[e]);
    }
    // ---- steering: foci with geometric delays; on folded axes some foci are mirror partners / on the axis (shared columns)
    const int F = S.nf;
    const bool whole_x = S.x_begin == 0 && S.x_count == S.n[0];
    const int mxf = (S.fold_x && whole_x) ? 2 : 1, myf = S.fold_y ? 2 : 1, n_img = mxf * myf;
    std::uniform_real_distribution<double> U(-4e-3, 4e-3), Z(20e-3, 40e-3);
    std::vector<double> foci(3 * (size_t)F);
    for (int f = 0; f < F; ++f) {
        double x = U(rng), y = U(rng), z = Z(rng);
        if (f % 5 == 0) { x = 0; y = 0; }                 // on the axis: all images share one vector
        else if (f % 5 == 1) x = 0;                       // on a symmetry plane
        else if (f % 5 == 2 && f >= 3) { x = -foci[3 * (size_t)(f - 1)]; y = foci[3 * (size_t)(f - 1) + 1]; z = foci[3 * (size_t)(f - 1) + 2]; }   // mirror partner of the previous focus
        foci[3 * (size_t)f] = x; foci[3 * (size_t)f + 1] = y; foci[3 * (size_t)f + 2] = z;
    }
    const double c0 = 1500.0, freq = 400e3;
    std::vector<double> delays((size_t)F * n), apod((size_t)F * n, 1.0);
    for (int f = 0; f < F; ++f) {
        double tmax = 0;
        std::vector<double> tof(n);
        for (int e = 0; e < n; ++e) {
            const double dx = foci[3 * (size_t)f] - pos[e], dy = foci[3 * (size_t)f + 1] - pos[(size_t)n + e], dz = foci[3 * (size_t)f + 2];
            tof[e] = std::sqrt(dx * dx + dy * dy + dz * dz) / c0; tmax = std::max(tmax, tof[e]);
        }
        for (int e = 0; e < n; ++e) delays[(size_t)f * n + e] = tmax - tof[e];
    }
    // mirror permutations of the element set (exact: lattice symmetric about 0)
    auto mirror = [&](int axis) {
        std::vector<int> p(n, -1);
        for (int e = 0; e < n; ++e)
            for (int o = 0; o < n; ++o)
                if (std::fabs(pos[(size_t)axis * n + o] + pos[(size_t)axis * n + e]) < 1e-12 && std::fabs(pos[(size_t)(1 - axis) * n + o] - pos[(size_t)(1 - axis) * n + e]) < 1e-12) p[e] = o;
        return p;
    };
    const std::vector<int> hpx = mirror(0), hpy = mirror(1);
    const std::vector<int> perm = mirror_perms(n, n_img, mxf == 2, myf == 2, hpx.data(), hpy.data(), 4);
    check_mirror_perms(perm, n, n_img, mxf == 2, myf == 2, hpx, hpy, 4);
    // ... the [nm][n] form of kernel 2b (no rows past the images), and both folds whatever this shape folds (the array is symmetric about 0 either way)
    check_mirror_perms(mirror_perms(n, n_img, mxf == 2, myf == 2, hpx.data(), hpy.data(), n_img), n, n_img, mxf == 2, myf == 2, hpx, hpy, n_img);
    check_mirror_perms(mirror_perms(n, 4, true, true, hpx.data(), hpy.data(), 4), n, 4, true, true, hpx, hpy, 4);
    Steering SV; SV.n = n; SV.F = F; SV.n_img = n_img; SV.perm = perm.data(); SV.delays = delays.data(); SV.apod = apod.data(); SV.area = area.data(); SV.freq = freq;
    for (int maxc : {32, 16, 8}) {
        Tiles tiles = pack_columns(SV, maxc);
        std::map<int, int> hits;
        for (auto& t : tiles) {
            CHECK((int)t.size() <= maxc && !t.empty(), "tile of %zu columns (max %d)", t.size(), maxc);
            for (auto& col : t) {
                ++g_columns;
                CHECK(col.ntgt >= 1 && col.ntgt <= 4, "column with %d targets", col.ntgt);
                for (int q = 0; q < 4; ++q) {
                    CHECK((q < col.ntgt) == (col.tgt[q] >= 0), "target list not dense");
                    if (col.tgt[q] < 0) continue;
                    hits[col.tgt[q]]++;
                    CHECK(ref_same_vector(SV, col.f, col.m, col.tgt[q] >> 2, col.tgt[q] & 3), "target %d stored by a column with another steering vector", col.tgt[q]);
                }
            }
        }
        for (int f = 0; f < F; ++f) for (int m = 0; m < n_img; ++m) CHECK(hits[f * 4 + m] == 1, "(focus %d, image %d) stored %d times (maxc %d)", f, m, hits[f * 4 + m], maxc);
        CHECK((int)hits.size() == F * n_img, "spurious targets");
        // sharing really happens: an on-axis focus on a doubly folded grid needs ONE column
        if (n_img == 4 && F >= 1) { int cnt = 0; for (auto& t : tiles) for (auto& col : t) if (col.f == 0) ++cnt; CHECK(cnt == 1, "on-axis focus in %d columns", cnt); }
        Tiles bal = tiles;
        balance_store_targets(bal, maxc);
        std::map<int, int> hits2;
        for (size_t t = 0; t < bal.size(); ++t) {
            CHECK((int)bal[t].size() <= maxc, "balanced tile overflows");
            for (auto& col : bal[t]) { for (int q = 0; q < col.ntgt; ++q) hits2[col.tgt[q]]++; if ((int)bal[t].size() < maxc) CHECK(col.ntgt <= 2, "unbalanced column although a slot is free"); }
        }
        CHECK(hits2 == hits, "balancing changed the target set");
        // store jobs of kernel 2e
        const std::vector<int> jobs = build_store_jobs(tiles, MFMA_MAX_NT, MFMA_COLS, COS_JOBS, true, true);
        for (size_t t = 0; t < tiles.size(); ++t)
            for (int nt = 0; nt < MFMA_MAX_NT; ++nt) {
                const int* jb = &jobs[(t * MFMA_MAX_NT + nt) * (COS_JOBS + 1)];
                std::multiset<int> want, got;
                for (int c16 = 0; c16 < 16; ++c16) {
                    const size_t o = (size_t)nt * MFMA_COLS + (c16 >> 1);
                    if (o < tiles[t].size()) for (int q = 0; q < tiles[t][o].ntgt; ++q) want.insert(c16 | ((tiles[t][o].tgt[q] & 3) << 4) | ((tiles[t][o].tgt[q] >> 2) << 6));
                }
                int cnt = 0;
                while (cnt < COS_JOBS && jb[cnt] >= 0) got.insert(jb[cnt++]);
                CHECK(got == want, "store jobs of tile %zu / %d", t, nt);
                CHECK((1 << jb[COS_JOBS]) >= cnt && (cnt <= 1 || (1 << (jb[COS_JOBS] - 1)) < cnt), "job count log2");
            }
    }
    // focus inference (flat array, geometric delays) ... and its refusal of anything else
    {
        std::vector<double> got;
        CHECK(infer_foci(true, n, F, pos.data(), delays.data(), c0, origin[2] + 0.5 * (S.n[2] - 1) * S.h, got), "geometric delays not recognised");
        for (size_t q = 0; q < got.size() && q < foci.size(); ++q) CHECK(std::fabs(got[q] - foci[q]) < 1e-6, "inferred focus off by %g", got[q] - foci[q]);
        std::vector<double> bad = delays;
        for (int e = 0; e < n; e += 3) bad[e] += 1e-7 * (1 + e % 5);
        CHECK(!infer_foci(true, n, F, pos.data(), bad.data(), c0, origin[2], got), "scrambled delays accepted");
    }
    // ---- block records of every shape the kernels use: (kxw, zb, limit) = 2g / 2e NT = 2 (3, 16, 40), 2e NT = 1 (6, 16, 0), 2e NT = 4 (2, 16, 0), 2f (8 | 16 | 24, 16, 0; positions one pitch apart),
    // each in every order of the records over the XCDs the host may choose (grp plane blocks -- or plane blocks x y cosets -- in a row on one XCD)
    struct Form { const char* name; int kxw, zb; unsigned grp; int max_pos; int xs; };
    std::vector<Form> forms;
    for (unsigned grp : {1u, 2u, 4u, 16u, 48u, 192u})
        for (const Form& f0 : {Form{"2g", 3, 16, 2, 40, 2}, Form{"2e nt1", 6, 16, 2, 0, 2}, Form{"2e nt4", 2, 16, 2, 0, 2}, Form{"2f", 8, 16, 2, 0, 1}, Form{"2f m2", 16, 16, 2, 0, 1}, Form{"2f m3", 24, 16, 2, 0, 1}}) {
            Form f = f0; f.grp = grp; forms.push_back(f);
        }
    for (const Form& fm : forms) {
        if (nt_force && fm.kxw != nt_force) continue;
        CosetParams Q{};
        Q.nx = S.x_count; Q.ny = S.n[1]; Q.nz = S.n[2]; Q.x_begin = S.x_begin;
        Q.x_lo = mxf == 2 ? Q.nx / 2 : 0; Q.y_lo = myf == 2 ? Q.ny / 2 : 0;
        Q.mx = L.mx; Q.my = L.my; Q.nsa = L.nsa; Q.nsb = L.nsb; Q.nsbp = (L.nsb + 1) & ~1; Q.xs = fm.xs;
        Q.ux0 = (int)std::llround((origin[0] - L.x0) / S.h); Q.uy0 = (int)std::llround((origin[1] - L.y0) / S.h);
        coset_partition(Q, fm.kxw, fm.zb);
        std::vector<CosetBlock> blk;
        std::string why;
        for (const bool heavy : {false, true}) {      // kernel 2g's records also with the position sets in the order of falling position count
            if (heavy && fm.max_pos == 0) continue;
            const bool ok = build_coset_blocks(Q, fm.zb, fm.grp, fm.max_pos, blk, why, heavy);
            CHECK(ok, "%s: %s", fm.name, why.c_str());
            if (!ok) continue;
            CHECK(blk.size() == (size_t)(Q.xs * Q.mx * Q.my * Q.nsx * Q.nsy * Q.kblocks), "record count");
            const int wx = Q.nx - Q.x_lo, wy = Q.ny - Q.y_lo;
            std::vector<unsigned char> cover((size_t)wx * wy * Q.kblocks, 0);
            for (const CosetBlock& B : blk) {
                if (B.npos <= 0) continue;
                ++g_records;
                CHECK(B.k0 % fm.zb == 0 && B.k0 >= 0 && B.k0 < Q.kblocks * fm.zb, "plane block %d", B.k0);
                CHECK(B.KX >= 1 && B.KX <= fm.kxw && B.KY >= 1 && B.KY <= COS_KYW && B.npos == B.KX * B.KY, "part %d x %d (npos %d)", B.KX, B.KY, B.npos);
                for (int pq = 0; pq < B.npos; ++pq) CHECK(((pq * B.ky_magic) >> 16) == pq / B.KY, "magic division %d / %d", pq, B.KY);
                for (int kx = 0; kx < B.KX; ++kx)
                    for (int ky = 0; ky < B.KY; ++ky) {
                        const int i = B.ibase + Q.xs * Q.mx * kx, j = B.jbase + Q.my * ky;
                        CHECK(i >= Q.x_lo && i < Q.nx && j >= Q.y_lo && j < Q.ny, "position (%d, %d) outside the computed region", i, j);
                        if (i >= Q.x_lo && i < Q.nx && j >= Q.y_lo && j < Q.ny) cover[((size_t)(i - Q.x_lo) * wy + (j - Q.y_lo)) * Q.kblocks + B.k0 / fm.zb]++;
                    }
            }
            size_t bad = 0;
            for (unsigned char v : cover) bad += v != 1;
            CHECK(bad == 0, "%s: %zu (voxel column, plane block) cells not covered exactly once (grid %dx%dx%d pitch %dx%d fold %d%d slab %d+%d)", fm.name, bad, S.n[0], S.n[1], S.n[2],
                  S.mxv, S.myv, mxf, myf, S.x_begin, S.x_count);
            // heaviest sets first: along every XCD's records (where a set's plane blocks stand in a row there, or every record is a set of its own) the position count never rises
            if (heavy && (fm.grp <= (unsigned)Q.kblocks || blk.size() % (8 * fm.grp) != 0)) {
                const bool rows = fm.grp <= (unsigned)Q.kblocks && (Q.kblocks % fm.grp) == 0 && blk.size() % (8 * fm.grp) == 0;
                if (rows && (unsigned)Q.kblocks == fm.grp) {
                    for (size_t id = 8; id < blk.size(); ++id) CHECK(blk[id].npos <= blk[id - 8].npos, "heaviest first: record %zu has %d positions behind %d", id, blk[id].npos, blk[id - 8].npos);
                } else if (!rows) {
                    for (size_t id = (size_t)Q.kblocks; id < blk.size(); ++id) CHECK(blk[id].npos <= blk[id - Q.kblocks].npos, "heaviest first: record %zu has %d positions behind %d", id, blk[id].npos, blk[id - Q.kblocks].npos);
                }
            }
            // the records that share z lines (plane blocks j, j + 1, ... of one part) sit 8 ids apart = one XCD (when the id space allows it)
            if (fm.grp >= 2 && fm.grp <= (unsigned)Q.kblocks && (Q.kblocks % fm.grp) == 0 && blk.size() % (8 * fm.grp) == 0)
                for (size_t id = 0; id + 8 < blk.size(); ++id)
                    if ((id / 8) % fm.grp != fm.grp - 1 && blk[id].npos > 0)
                        CHECK(blk[id + 8].ibase == blk[id].ibase && blk[id + 8].jbase == blk[id].jbase && blk[id + 8].k0 == blk[id].k0 + fm.zb, "line partners not 8 ids apart");
        }
    }
    // ---- the decision over this lattice: 1 .. 64 foci, plain and complex output, and once with a per-term factor (the fallback to kernels 2a-d)
    Geometry G{n, pos.data(), area.data(), hpx.data(), hpy.data(), {origin[0], origin[1], origin[2]}, S.h, {S.n[0], S.n[1], S.n[2]}, S.x_begin, S.x_count, mxf, myf, &L};
    for (int Fd : {1, 3, 8, 9, 64})
        for (int variation = 0; variation < (Fd == 3 ? 3 : 2); ++variation) check_decision(G, Fd, variation == 1, variation == 2);
}

// ---- decide_variant: what nobody checks on a GPU -- the flags imply each other, NT covers the widest tile, the tables have the sizes the kernels
// index them with, the pair tables of the NT <= 2 shapes have an even row count, the fallback leaves no per-term factor with a kernel that cannot
// carry it, and the record key determines the block records
static std::map<std::vector<int>, std::vector<CosetBlock>> g_records_of_key;
static std::map<std::string, int> g_decided;      // kernel name -> decisions that chose it
static void check_decision(const Geometry& G, int F, bool cplx, bool absorb) {
    const int n = G.n;
    std::mt19937_64 rng(1000003ull * n + 131 * F + G.gn[2]);      // (a stream of its own: the shapes stay the ones each seed always drew)
    std::uniform_real_distribution<double> U(-4e-3, 4e-3), Z(20e-3, 40e-3);
    std::vector<double> foci(3 * (size_t)F), delays((size_t)F * n), apod((size_t)F * n, 1.0);
    for (int f = 0; f < F; ++f) {
        double x = U(rng), y = U(rng), z = Z(rng);
        if (f % 5 == 0) { x = 0; y = 0; }                 // on the axis: all images share one vector
        else if (f % 5 == 2 && f >= 3) { x = -foci[3 * (size_t)(f - 1)]; y = foci[3 * (size_t)(f - 1) + 1]; z = foci[3 * (size_t)(f - 1) + 2]; }   // mirror partner of the previous focus
        foci[3 * (size_t)f] = x; foci[3 * (size_t)f + 1] = y; foci[3 * (size_t)f + 2] = z;
        double tmax = 0;
        for (int e = 0; e < n; ++e) {
            const double dx = x - G.pos[e], dy = y - G.pos[(size_t)n + e];
            delays[(size_t)f * n + e] = std::sqrt(dx * dx + dy * dy + z * z) / 1500.0; tmax = std::max(tmax, delays[(size_t)f * n + e]);
        }
        for (int e = 0; e < n; ++e) delays[(size_t)f * n + e] = tmax - delays[(size_t)f * n + e];
    }
    VariantIn in;
    in.n = n; in.F = F; in.pos = G.pos; in.area = G.area; in.delays = delays.data(); in.apod = apod.data(); in.px = G.px; in.py = G.py; in.foci = foci.data();
    in.freq = 400e3; in.c = 1500.0; in.p0_pa = 1e5; in.x_begin = G.x_begin; in.x_count = G.x_count;
    for (int a = 0; a < 3; ++a) { in.origin[a] = G.origin[a]; in.spacing[a] = G.h; in.gn[a] = G.gn[a]; }
    in.flags = FLAG_OUT_PMAG | FLAG_OUT_INTENSITY | (cplx ? FLAG_OUT_COMPLEX : 0u);
    const double rev = in.freq / in.c;
    FieldParams& P = in.fp;
    P.nx = G.x_count; P.ny = G.gn[1]; P.nz = G.gn[2]; P.n_el = n; P.x_begin = G.x_begin; P.hx = P.hy = P.hz = (float)(G.h * rev);
    P.dmin2 = (float)(0.25 * G.h * G.h * rev * rev); P.inten_scale = 1e-10f; P.flat_ez = (float)(-G.origin[2] * rev); P.vox = (long long)P.nx * P.ny * P.nz; P.flags = in.flags & 7u;
    in.flat = true; in.min_dist = G.origin[2];      // (the grid starts 4 mm above the array: neither clamp nor near)
    in.mx = G.mx; in.my = G.my; in.lat = G.L;
    if (absorb) { in.absorb_np_m = 5.0; in.dir_lattice = true; }
    std::vector<double> nf_s2;
    int slot_rows = G.L->nsbp;
    const VariantPlan p = decide_variant(in, nf_s2, slot_rows);
    const char* v = p.variant.c_str();
    ++g_decided[p.variant.substr(0, p.variant.find('<'))];
    CHECK(!p.variant.empty() && p.variant.size() < 383, "decision: variant string of %zu characters", p.variant.size());
    CHECK((!p.use_toep || p.use_coset) && (!p.use_cosetp || p.use_coset) && (!p.use_coset || p.use_lattice) && (!p.use_lattice || p.use_mfma) && !(p.use_toep && p.use_cosetp),
          "decision: family flags contradict each other (%s)", v);
    CHECK(!p.fp8corr || (p.use_coset && cos_fp8(p.nt)), "decision: e4m3 products with NT = %d / without a coset kernel (%s)", p.nt, v);
    CHECK(!(in.modifier() && p.use_mfma && !(p.use_lattice && p.use_coset)), "decision: a per-term factor left with a kernel that carries none (%s)", v);
    CHECK(in.modifier() || (p.allow_shared && p.mx == in.mx && p.my == in.my), "decision: folds changed without a fallback (%s)", v);
    if (!p.use_mfma) { CHECK(p.tiles.empty() && p.colinfo.empty() && p.jobs.empty(), "decision: column tables without a matrix kernel (%s)", v); return; }
    int widest = 0, cols = 0;
    for (const auto& t : p.tiles) { widest = std::max(widest, (int)t.size()); cols += (int)t.size(); }
    CHECK((p.nt == 1 || p.nt == 2 || p.nt == 4) && p.nt * MFMA_COLS >= widest && widest >= 1, "decision: tile of %d columns exceeds NT = %d (%s)", widest, p.nt, v);
    CHECK((p.use_cosetp ? cols >= p.total_cols : cols == p.total_cols) && p.mp.n_tiles == (int)p.tiles.size(), "decision: %d columns counted, %d packed", p.total_cols, cols);      // (kernel 2g: balancing hands store targets to free slots)
    // colinfo as mfma_pack_k and the kernels index it: [tile][32 columns][f, m], then [tile][32 columns][4 targets]
    constexpr int MAXC = MFMA_COLS * MFMA_MAX_NT;
    const size_t n_col = p.tiles.size() * MAXC;
    CHECK(p.colinfo.size() == n_col * 6 && p.perm.size() == 4 * (size_t)n, "decision: colinfo of %zu entries for %zu tiles, %zu permutation entries", p.colinfo.size(), p.tiles.size(), p.perm.size());
    if (p.colinfo.size() == n_col * 6)
        for (size_t t = 0; t < p.tiles.size(); ++t)
            for (size_t o = 0; o < (size_t)MAXC; ++o) {
                const int* fm = &p.colinfo[(t * MAXC + o) * 2]; const int* tg = &p.colinfo[n_col * 2 + (t * MAXC + o) * 4];
                if (o < p.tiles[t].size()) CHECK(fm[0] == p.tiles[t][o].f && fm[1] == p.tiles[t][o].m && std::equal(tg, tg + 4, p.tiles[t][o].tgt), "decision: colinfo of tile %zu column %zu", t, o);
                else CHECK(fm[0] == -1 && fm[1] == -1 && tg[0] == -1, "decision: colinfo names a column past the tile (%zu, %zu)", t, o);
            }
    CHECK(p.n_pad % 16 == 0 && p.n_pad >= n && p.mp.n_el_pad == p.n_pad, "decision: %d padded elements for %d", p.n_pad, n);
    CHECK(p.g_scale > 0 && p.out_scale > 0 && p.mfma_wscale > 0 && std::isfinite(p.mfma_wscale), "decision: operand scales");
    if (!p.use_lattice) return;
    CHECK(slot_rows == p.lp.nsbp && p.n_pad == G.L->nsa * slot_rows * 64 && (slot_rows == G.L->nsb || slot_rows == ((G.L->nsb + 1) & ~1)), "decision: %d rows of the slot map (nsb %d)", slot_rows, G.L->nsb);
    if (!p.use_coset) { CHECK(p.jobs.empty(), "decision: store jobs without a coset kernel"); return; }
    const CosetParams& Q = p.cp;
    CHECK(p.jobs.size() == p.tiles.size() * MFMA_MAX_NT * (COS_JOBS + 1), "decision: %zu store-job entries for %zu tiles", p.jobs.size(), p.tiles.size());
    CHECK(Q.nsbp == slot_rows && (p.nt > 2 || Q.nsbp % 2 == 0), "decision: NT = %d with %d rows of pair tables", p.nt, Q.nsbp);
    CHECK(Q.xs == (p.use_toep ? 1 : 2) && Q.n_foci == F && Q.kblocks == (Q.nz + COS_ZB - 1) / COS_ZB, "decision: coset parameters");
    CHECK(!p.use_toep || (p.total_cols == 1 && p.toep.nm >= 1 && p.toep.nm <= TOEP_MAX_NM), "decision: kernel 2f with %d columns, %d row tiles", p.total_cols, p.toep.nm);
    // the record key: it names every quantity build_coset_blocks reads, and plans with one key have the same records (what the caller's cache relies on)
    const int kcut = p.fp8corr ? p.fp8_kcut : 0;
    const int key[17] = {Q.nx, Q.ny, Q.nz, Q.x_lo, Q.y_lo, Q.mx, Q.my, Q.nsx, Q.nsy, Q.kblocks, COS_ZB, (int)p.kgrp, p.use_cosetp ? 40 : 0, Q.xs, kcut, (int)p.kgrp_near, p.use_cosetp ? 1 : 0};      // (kernel 2g: its position sets heaviest first)
    CHECK(std::equal(key, key + 17, p.rec_key), "decision: the record key misses a quantity the block records depend on (%s)", v);
    CHECK(p.heavy_first == p.use_cosetp, "decision: heaviest sets first is kernel 2g's order and no other kernel's (%s)", v);
    std::vector<CosetBlock> blk;
    std::string why;
    const bool ok = build_variant_blocks(p, blk, why);
    CHECK(ok, "decision: block records refused: %s", why.c_str());
    if (!ok) return;
    CHECK(blk.size() == (size_t)Q.xs * Q.mx * Q.my * Q.nsx * Q.nsy * Q.kblocks && p.blocks_near <= blk.size() && p.blocks_near == (size_t)Q.xs * Q.mx * Q.my * Q.nsx * Q.nsy * (kcut / COS_ZB),
          "decision: %zu block records, %u below the cut", blk.size(), p.blocks_near);
    const auto hit = g_records_of_key.emplace(std::vector<int>(p.rec_key, p.rec_key + 17), blk);
    if (!hit.second) CHECK(hit.first->second.size() == blk.size() && !memcmp(hit.first->second.data(), blk.data(), blk.size() * sizeof(CosetBlock)), "decision: two plans with one record key, different block records (%s)", v);
}

// ---- e4m3 error rule (olx_plan.h: fp8_first_plane, fp8_split_pays, nearfield_s2) on BASELINE's 16 x 16 @ 3 mm array, uniform drive ----
struct Fp8Case {
    int na = 16;                               // na x na elements @ 3 mm
    double h = 0.25e-3, z0 = 5e-3; int nxy = 256, nz = 256;
    double shift = 0;                          // lateral shift of the grid [voxels]
    int x_begin = 0, x_count = -1;             // slab (-1: the whole grid)
    std::vector<double> foci;                  // [F][3]
    double taper = 0;                          // apodization exp(-taper r^2 / r_max^2)
};
static std::vector<double> wheel8() {          // the 8-focus wheel: (0, 0, 40) mm and seven spokes of 5 mm
    std::vector<double> f = {0, 0, 40e-3};
    for (int i = 0; i < 7; ++i) { f.push_back(5e-3 * std::cos(2 * M_PI * i / 7)); f.push_back(5e-3 * std::sin(2 * M_PI * i / 7)); f.push_back(40e-3); }
    return f;
}
struct Fp8Result { int cut, restated; double neff_min; int planes; };
// fp8_first_plane on the case, twice (empty and filled cache), next to the checker's own restatement of the rule: every focus inside the slab,
// N_eff >= 255.5, FP8_ERR_K (1 + planes / 4) wmax sqrt(S2 of the planes from the cut on) <= FP8_ERR_BOUND peak -- nearfield_s2 asked afresh per plane block
static Fp8Result run_fp8_case(const Fp8Case& c, const char* what) {
    const int na = c.na, n = na * na, F = (int)c.foci.size() / 3;
    std::vector<double> pos(3 * (size_t)n, 0.0), area(n, 7.29e-6), apod((size_t)F * n);
    const double rmax2 = 2 * std::pow(0.5 * (na - 1) * 3e-3, 2);
    for (int a = 0; a < na; ++a) for (int b = 0; b < na; ++b) {
        const int e = a * na + b;
        pos[e] = (a - 0.5 * (na - 1)) * 3e-3; pos[(size_t)n + e] = (b - 0.5 * (na - 1)) * 3e-3;
        for (int f = 0; f < F; ++f) apod[(size_t)f * n + e] = std::exp(-c.taper * (pos[e] * pos[e] + pos[(size_t)n + e] * pos[(size_t)n + e]) / rmax2);
    }
    const double origin[3] = {(-(c.nxy - 1) / 2.0 + c.shift) * c.h, (-(c.nxy - 1) / 2.0 + c.shift) * c.h, c.z0}, spacing[3] = {c.h, c.h, c.h};
    const int gn[3] = {c.nxy, c.nxy, c.nz}, xb = c.x_begin, xc = c.x_count < 0 ? c.nxy : c.x_count;
    const double lo[3] = {origin[0] + xb * c.h, origin[1], origin[2]}, hi[3] = {origin[0] + (xb + xc - 1) * c.h, origin[1] + (c.nxy - 1) * c.h, origin[2] + (c.nz - 1) * c.h};
    Lattice L;
    detect_lattice(L, true, n, pos.data(), spacing, lo, hi, 0.5 * c.h);
    CHECK(L.ok && L.ax == na && L.ay == na, "fp8 rule (%s): lattice not recognised", what);
    Fp8Result R{-1, -1, 1e300, 0};
    if (!L.ok) return R;
    std::vector<double> cache;
    R.cut = fp8_first_plane(n, pos.data(), area.data(), apod.data(), F, c.foci.data(), origin, spacing, gn, xb, xc, L, cache);
    const std::vector<double> filled = cache;
    const int again = fp8_first_plane(n, pos.data(), area.data(), apod.data(), F, c.foci.data(), origin, spacing, gn, xb, xc, L, cache);
    CHECK(again == R.cut && cache == filled, "fp8 rule (%s): plane %d with the filled cache, %d without", what, again, R.cut);
    // the restatement
    bool ok = true;
    double worst = 0;      // max_f wmax_f / peak_f
    for (int f = 0; f < F; ++f) {
        const double* fo = &c.foci[3 * (size_t)f];
        if (fo[0] < lo[0] - 0.5 * c.h || fo[0] > hi[0] + 0.5 * c.h || fo[1] < lo[1] - 0.5 * c.h || fo[1] > hi[1] + 0.5 * c.h || fo[2] < lo[2] - 0.5 * c.h || fo[2] > hi[2] + 0.5 * c.h) ok = false;
        double s1 = 0, s2 = 0, wmax = 0, peak = 0;
        for (int e = 0; e < n; ++e) {
            const double w = apod[(size_t)f * n + e] * area[e];
            s1 += w; s2 += w * w; wmax = std::max(wmax, w);
            peak += w / std::sqrt(std::pow(fo[0] - pos[e], 2) + std::pow(fo[1] - pos[(size_t)n + e], 2) + fo[2] * fo[2]);
        }
        R.neff_min = std::min(R.neff_min, s1 * s1 / s2);
        worst = std::max(worst, wmax / peak);
    }
    if (R.neff_min < 255.5) ok = false;
    // the array is centred on 0: its symmetry planes are x = 0 and y = 0; a plane carries voxels when 0 is a voxel coordinate of the slab
    for (int a = 0; a < 2; ++a) {
        const double idx = -origin[a] / c.h;
        const int b0 = a == 0 ? xb : 0, cnt = a == 0 ? xc : c.nxy;
        if (std::fabs(idx - std::round(idx)) < 1e-6 && idx > b0 - 0.5 && idx < b0 + cnt - 0.5) ++R.planes;
    }
    if (ok)
        for (int k = 0; k < c.nz && R.restated < 0; k += COS_ZB) {
            const int b0[3] = {xb, 0, k}, cnt[3] = {xc, c.nxy, c.nz - k};
            const double s2 = nearfield_s2(n, pos.data(), origin, spacing, b0, cnt, 0.5 * c.h);
            if (k / COS_ZB < (int)filled.size() && filled[k / COS_ZB] >= 0) CHECK(filled[k / COS_ZB] == s2, "fp8 rule (%s): cached S2 of plane block %d differs from nearfield_s2", what, k / COS_ZB);
            if (FP8_ERR_K * (1.0 + 0.25 * R.planes) * worst * std::sqrt(s2) <= FP8_ERR_BOUND) R.restated = k;
        }
    CHECK(R.cut == R.restated, "fp8 rule (%s): fp8_first_plane gives plane %d, the restated rule plane %d (N_eff %.1f, %d symmetry plane(s) with voxels)", what, R.cut, R.restated, R.neff_min, R.planes);
    return R;
}

// Known decisions (the cut planes are what the rule computes; DESIGN 5.2 quotes them), one case per way the rule refuses, and nearfield_s2 against
// the brute-force maximum over every voxel of the grid's first planes (ratios from tools/emul_fp8_bound.py).
static void check_fp8_rule() {
    const int na = 16, n = na * na;
    std::vector<double> pos(3 * (size_t)n, 0.0);
    for (int a = 0; a < na; ++a) for (int b = 0; b < na; ++b) { pos[(size_t)a * na + b] = (a - 7.5) * 3e-3; pos[(size_t)n + a * na + b] = (b - 7.5) * 3e-3; }
    double peak = 0;
    for (int e = 0; e < n; ++e) peak += 1.0 / std::sqrt(pos[e] * pos[e] + pos[(size_t)n + e] * pos[(size_t)n + e] + 40e-3 * 40e-3);
    // cut1 / cut8: first plane of the e4m3 products with the on-axis focus (0, 0, 40) mm / the 8-focus wheel; pays1 / pays8: fp8_split_pays at that cut
    struct G { double h, z0; int nxy, nz; double ratio; int cut1, cut8; bool pays1, pays8; } grids[] = {
        {0.25e-3, 5e-3, 256, 256, 0.188, 0, 0, true, true},             // the headline grid
        {0.5e-3, 5e-3, 128, 128, 0.188, 0, 0, true, true},              // configs[1]
        {1e-3, -4e-3, 61, 65, 0.340, 32, 32, false, false},             // the reference's default SimSetup: through the element plane
        {0.5e-3, -4e-3, 121, 129, 0.730, 48, 48, false, false},          // (odd counts: a voxel sits ON every element -- the clamp distance -- and on both symmetry planes)
        {0.25e-3, -4e-3, 241, 257, 1.403, 80, 80, false, false},
        {0.25e-3, 0.25e-3, 256, 256, 0.61, 16, 16, true, true},      // one voxel above the element plane
        {0.25e-3, 1e-3, 256, 256, 0.285, 16, 16, true, true},
        {0.5e-3, 0.5e-3, 128, 128, 0.0, 16, 16, false, true},         // ... on a grid below 8 M (voxel, focus) pairs with one focus
    };
    for (const G& g : grids) {
        const double origin[3] = {-(g.nxy - 1) / 2.0 * g.h, -(g.nxy - 1) / 2.0 * g.h, g.z0}, spacing[3] = {g.h, g.h, g.h};
        const int b0[3] = {0, 0, 0}, cnt[3] = {g.nxy, g.nxy, g.nz};
        const double s2 = nearfield_s2(n, pos.data(), origin, spacing, b0, cnt, 0.5 * g.h);
        const double ratio = std::sqrt(s2) / peak;
        if (g.ratio > 0) CHECK(std::fabs(ratio - g.ratio) <= 0.03 * g.ratio + 0.005, "fp8 rule: ratio %.4f, expected %.3f (h %.2g z0 %.2g)", ratio, g.ratio, g.h, g.z0);
        // the rule itself: on-axis focus and the 8-focus wheel
        Fp8Case c; c.h = g.h; c.z0 = g.z0; c.nxy = g.nxy; c.nz = g.nz;
        for (int F : {1, 8}) {
            c.foci = F == 1 ? std::vector<double>{0, 0, 40e-3} : wheel8();
            const Fp8Result R = run_fp8_case(c, F == 1 ? "known grid, on-axis focus" : "known grid, 8-focus wheel");
            const int want = F == 1 ? g.cut1 : g.cut8;
            if (R.planes > 0 && want > 0) CHECK(R.cut == want, "fp8 rule, symmetry-plane factor: h %.2g z0 %.2g (voxels on %d symmetry planes), %d foci: first plane %d, expected %d", g.h, g.z0, R.planes, F, R.cut, want);
            else CHECK(R.cut == want, "fp8 rule: h %.2g z0 %.2g, %d foci: first plane %d, expected %d", g.h, g.z0, F, R.cut, want);
            if (R.cut > 0) {
                CHECK(R.cut % COS_ZB == 0, "fp8 rule: cut %d is no multiple of the plane block", R.cut);
                const bool pays = fp8_split_pays(g.nxy, g.nxy, g.nz, F, R.cut);
                CHECK(pays == (F == 1 ? g.pays1 : g.pays8), "fp8 rule: h %.2g z0 %.2g, %d foci: a split at plane %d pays = %d, expected %d", g.h, g.z0, F, R.cut, (int)pays, (int)(F == 1 ? g.pays1 : g.pays8));
            }
        }
        if (g.ratio <= 0) continue;
        // brute force over the three planes nearest to the elements (a quadrant: the array and the grid are symmetric)
        double brute = 0;
        int kn = (int)std::llround((0.0 - g.z0) / g.h); kn = std::max(0, std::min(kn, g.nz - 1));
        for (int k = std::max(0, kn - 1); k <= std::min(g.nz - 1, kn + 1); ++k)
            for (int i = g.nxy / 2; i < g.nxy; ++i)
                for (int j = g.nxy / 2; j < g.nxy; ++j) {
                    const double x = origin[0] + i * g.h, y = origin[1] + j * g.h, z = origin[2] + k * g.h;
                    double sum = 0;
                    for (int e = 0; e < n; ++e) {
                        const double dx = x - pos[e], dy = y - pos[(size_t)n + e];
                        sum += 1.0 / std::max(dx * dx + dy * dy + z * z, 0.25 * g.h * g.h);
                    }
                    brute = std::max(brute, sum);
                }
        CHECK(s2 <= brute * (1 + 1e-12) && s2 >= 0.97 * brute, "nearfield_s2 %.6g vs brute-force maximum %.6g (h %.2g z0 %.2g)", s2, brute, g.h, g.z0);
    }
    // the split condition alone: 8 M (voxel, focus) pairs above the cut, and at least three quarters of the planes above it
    CHECK(fp8_split_pays(121, 121, 129, 8, 32) && !fp8_split_pays(121, 121, 129, 1, 32) && !fp8_split_pays(61, 61, 65, 8, 32), "fp8 rule: split condition, pairs above the cut");
    CHECK(fp8_split_pays(256, 256, 256, 8, 64) && !fp8_split_pays(256, 256, 256, 8, 80) && !fp8_split_pays(241, 241, 257, 8, 80), "fp8 rule: split condition, planes above the cut");
    // ---- one case per way the rule refuses
    {   // a focus half a voxel outside the slab along x: refused there, admitted in the slab that holds it
        Fp8Case c; c.foci = {0.125e-3, 0, 40e-3};      // slab [0, 128) ends at x = 0 (its last voxel's upper face)
        c.x_begin = 0; c.x_count = 128;
        CHECK(run_fp8_case(c, "focus outside the slab").cut == -1, "fp8 rule, focus inside the slab: a focus half a voxel outside along x admitted");
        c.x_begin = 128;
        CHECK(run_fp8_case(c, "focus inside the slab").cut >= 0, "fp8 rule, focus inside the slab: the slab that holds the focus refused");
    }
    {   // 15 x 15 elements: N_eff = 225
        Fp8Case c; c.na = 15; c.foci = {0, 0, 40e-3};
        const Fp8Result R = run_fp8_case(c, "15 x 15 elements");
        CHECK(R.cut == -1 && std::fabs(R.neff_min - 225.0) < 1e-6, "fp8 rule, N_eff threshold: 15 x 15 equally driven elements (N_eff %.1f < 255.5) admitted from plane %d", R.neff_min, R.cut);
    }
    {   // a strongly tapered apodization on 16 x 16
        Fp8Case c; c.taper = 3.0; c.foci = {0, 0, 40e-3};
        const Fp8Result R = run_fp8_case(c, "tapered apodization");
        CHECK(R.cut == -1 && R.neff_min < 255.5, "fp8 rule, N_eff threshold: tapered drive (N_eff %.1f) admitted from plane %d", R.neff_min, R.cut);
        c.taper = 1e-4;      // ... and a taper that leaves N_eff at 256 to within the threshold's margin is admitted
        const Fp8Result R2 = run_fp8_case(c, "barely tapered apodization");
        CHECK(R2.cut == 0 && R2.neff_min >= 255.5 && R2.neff_min < 256.0, "fp8 rule, N_eff threshold: barely tapered drive (N_eff %.3f) refused (%d)", R2.neff_min, R2.cut);
    }
    for (const G& g : grids) {   // the grids through the element plane shifted by half a voxel laterally: no voxel on a symmetry plane
        if (!(g.z0 < 0)) continue;
        Fp8Case c; c.h = g.h; c.z0 = g.z0; c.nxy = g.nxy; c.nz = g.nz; c.foci = {0, 0, 40e-3};
        const Fp8Result ctr = run_fp8_case(c, "centred odd grid");
        c.shift = 0.5;
        const Fp8Result sh = run_fp8_case(c, "grid shifted by half a voxel");
        CHECK(ctr.planes == 2 && sh.planes == 0 && sh.cut >= 0 && sh.cut <= ctr.cut, "fp8 rule, symmetry-plane factor: h %.2g: centred (%d planes with voxels) from plane %d, shifted (%d) from plane %d",
              g.h, ctr.planes, ctr.cut, sh.planes, sh.cut);
    }
    {   // a slab beside the array sees the clamped nearest voxel, not the element's own position
        const double origin[3] = {-31.875e-3, -31.875e-3, 5e-3}, spacing[3] = {0.25e-3, 0.25e-3, 0.25e-3};
        const int b0[3] = {192, 0, 0}, cnt[3] = {64, 256, 256}, whole0[3] = {0, 0, 0}, whole[3] = {256, 256, 256};
        CHECK(nearfield_s2(n, pos.data(), origin, spacing, b0, cnt, 0.125e-3) < nearfield_s2(n, pos.data(), origin, spacing, whole0, whole, 0.125e-3), "slab beside the centre must see a smaller sum");
    }
}

// ---- kernel 2f's block shape (toep_plan): known shapes of the project and invariants over fuzzed widths
static int popcount(unsigned v) { int c = 0; for (; v; v &= v - 1) ++c; return c; }
static void check_toep_plan(std::mt19937_64& rng) {
    auto ri = [&](int lo, int hi) { return (int)(lo + rng() % (unsigned long long)(hi - lo + 1)); };
    // 16-wide arrays: one column of 16; two row tiles where a part holds more than 8 x positions (kx positions of a coset along x, cut into parts of <= 16)
    for (int kx = 1; kx <= 40; ++kx) {
        const ToepPlan T = toep_plan(16, 3, 3, 1, 3 * kx, 60, 64, false);
        const int parts = std::max(1, (kx + 15) / 16), per_part = (kx + parts - 1) / parts;
        CHECK(T.saw == 16 && T.nsa == 1 && T.nm == (per_part > 8 ? 2 : 1) && T.kyw == ToepShape<1>::KYW && T.ks_mask == 3u && T.ksteps_total == 2 && T.e4_units == 2,
              "toep_plan: 16-wide array, %d x positions: saw %d nsa %d nm %d kyw %d mask %x", kx, T.saw, T.nsa, T.nm, T.kyw, T.ks_mask);
    }
    {   // the headline array with one on-axis focus (16 x 16 @ 12 voxels, 256^3 folded: 11 x positions) and configs[1] (6 voxels, 128^3: 11)
        CHECK(toep_plan(16, 12, 12, 1, 128, 128, 256, false).nm == 2 && toep_plan(16, 6, 6, 1, 64, 64, 128, false).nm == 2 && toep_plan(16, 6, 6, 1, 32, 32, 48, false).nm == 1, "toep_plan: BASELINE's 16 x 16 array");
    }
    {   // BASELINE configs[3]: 32 x 32 @ 12 voxels on 512^3 (folded: 256 x 256 computed voxels)
        const ToepPlan T = toep_plan(32, 12, 12, 1, 256, 256, 512, false);
        CHECK(T.saw == 24 && T.nsa == 2 && T.nm == 3 && T.kyw == ToepShape<3>::KYW, "toep_plan: configs[3]: saw %d nsa %d nm %d kyw %d", T.saw, T.nsa, T.nm, T.kyw);
        CHECK(T.ks_mask == (3u | (2u << 2)) && T.ksteps_total == 3 && T.e4_units == 3, "toep_plan: configs[3]: mask %x (the second column fills K-step 1 only), %d K-steps, %d e4m3 units", T.ks_mask, T.ksteps_total, T.e4_units);
        const ToepPlan D = toep_plan(32, 12, 12, 1, 256, 256, 512, true);      // the DIR instantiations have no three-tile shape
        CHECK(D.nm == 1 && D.kyw == ToepShape<1>::KYW && D.ks_mask == T.ks_mask && D.e4_units == 4, "toep_plan: configs[3] with per-term factors: nm %d", D.nm);
        const ToepPlan P1 = toep_plan(32, 12, 12, 1, 256, 256, 512, false, 0, 1), P16 = toep_plan(32, 12, 12, 1, 256, 256, 512, false, 16, 0);      // the A/B pins
        CHECK(P1.nm == 1 && P1.saw == 24 && P16.saw == 16 && P16.nsa == 2 && P16.nm == 2 && P16.ks_mask == 0xfu, "toep_plan: pins: nm %d / saw %d nsa %d nm %d mask %x", P1.nm, P16.saw, P16.nsa, P16.nm, P16.ks_mask);
    }
    {   // a 20-wide array (20 x 20 @ 6 voxels on 206 x 206 x 320, folded): one column of 20, three row tiles; on a small grid (fewer than 256 blocks) one
        const ToepPlan T = toep_plan(20, 6, 6, 1, 103, 103, 320, false), S = toep_plan(20, 6, 6, 1, 36, 36, 40, false);
        CHECK(T.saw == 20 && T.nsa == 1 && T.nm == 3 && T.kyw == ToepShape<3>::KYW && T.ks_mask == 3u && T.ksteps_total == 2 && T.e4_units == 2, "toep_plan: 20-wide array: saw %d nsa %d nm %d mask %x", T.saw, T.nsa, T.nm, T.ks_mask);
        CHECK(S.saw == 20 && S.nm == 1, "toep_plan: 20-wide array on a small grid: nm %d", S.nm);
    }
    {   // more than 16 super-block columns: reported through nsa, no masks (the caller fails)
        const ToepPlan T = toep_plan(400, 2, 2, 1, 100, 100, 32, false);
        CHECK(T.saw == 24 && T.nsa == 17 && T.ks_mask == 0u && T.ksteps_total == 0, "toep_plan: 400-wide array: nsa %d mask %x", T.nsa, T.ks_mask);
    }
    for (int k = 0; k < 2000; ++k) {
        const int ax = ri(4, 40), xs = ri(1, 2), mx = ri(1, 12), my = ri(1, 12), wx = ri(1, 300), wy = ri(1, 300), nz = ri(1, 520), saw_pin = rng() % 4 ? 0 : ri(8, 24), nm_pin = rng() % 8 ? 0 : (rng() & 1 ? 3 : 1);
        const ToepPlan T = toep_plan(ax, mx, my, xs, wx, wy, nz, rng() % 4 == 0, saw_pin, nm_pin);
        bool ok = T.saw >= 1 && T.saw <= TOEP_SA_MAX && T.nsa >= 1 && T.nsa * T.saw >= ax && (T.nsa - 1) * T.saw < ax && T.nm >= 1 && T.nm <= TOEP_MAX_NM && T.kyw >= 1 && T.kyw <= COS_KYW;
        ok = ok && (T.nm != 2 || T.saw + 15 <= 32);      // two row tiles read the second tile 8 columns on in 32-word rows
        for (int sa = 0; ok && sa < T.nsa; ++sa) ok = ((T.ks_mask >> (2 * sa)) & 3u) != 0;
        ok = ok && (T.nsa >= 16 || (T.ks_mask >> (2 * T.nsa)) == 0) && T.ksteps_total == popcount(T.ks_mask) && T.e4_units >= T.nsa && T.e4_units <= 2 * T.nsa;
        CHECK(ok, "toep_plan(ax %d, pitch %dx%d, xs %d, %dx%dx%d, pins %d %d): saw %d nsa %d nm %d kyw %d mask %x, %d K-steps, %d e4m3 units", ax, mx, my, xs, wx, wy, nz, saw_pin, nm_pin,
              T.saw, T.nsa, T.nm, T.kyw, T.ks_mask, T.ksteps_total, T.e4_units);
    }
}

int main(int argc, char** argv) {
    check_fp8_rule();
    const int cases = argc > 1 ? atoi(argv[1]) : 200;
    const unsigned long long seed = argc > 2 ? strtoull(argv[2], nullptr, 10) : 147;
    std::mt19937_64 rng(seed);
    {
        std::mt19937_64 rng2(seed);      // (a stream of its own: the shapes below stay the ones each seed always drew)
        check_toep_plan(rng2);
    }
    auto ri = [&](int lo, int hi) { return (int)(lo + rng() % (unsigned long long)(hi - lo + 1)); };
    int done = 0;
    // BASELINE's shapes first: 16 x 16 @ 12 voxels on 256^3 (8-focus shard, 64-focus sweep, 4-GPU x-slab), 32 x 32 @ 12 on 512^3 (coarse: plane count cut)
    const Shape fixed[] = {{16, 16, 12, 12, {256, 256, 256}, 0, 256, true, true, 8, 0.25e-3}, {16, 16, 12, 12, {256, 256, 256}, 0, 256, true, true, 64, 0.25e-3},
                           {16, 16, 12, 12, {256, 256, 256}, 64, 64, true, true, 8, 0.25e-3}, {32, 32, 12, 12, {512, 512, 48}, 0, 512, true, true, 1, 0.125e-3},
                           {16, 16, 6, 6, {128, 128, 128}, 0, 128, true, true, 1, 0.5e-3}, {8, 8, 4, 4, {61, 61, 65}, 0, 61, true, true, 4, 1e-3}};
    for (const Shape& S : fixed) { check_shape(S, rng, 0); ++done; }
    for (int k = 0; k < cases; ++k) {
        Shape S{};
        S.nax = ri(4, 20); S.nay = ri(4, 20); S.mxv = ri(1, 12); S.myv = ri(1, 12);
        S.n[0] = ri(9, 140); S.n[1] = ri(9, 140); S.n[2] = ri(3, 70);
        S.fold_x = rng() & 1; S.fold_y = rng() & 1;
        if (rng() % 4 == 0) { S.x_begin = ri(0, S.n[0] / 2); S.x_count = ri(1, S.n[0] - S.x_begin); } else { S.x_begin = 0; S.x_count = S.n[0]; }
        S.nf = ri(1, 20); S.h = 0.5e-3;
        check_shape(S, rng, 0);
        ++done;
    }
    printf("plan_check: decisions");
    for (const auto& kv : g_decided) printf(" %s x%d", kv.first.c_str(), kv.second);
    printf("\n");
    printf("plan_check: %d shapes (%lld recognised lattices, %lld columns, %lld block records), %d violations\n", done, g_lattices, g_columns, g_records, g_fail);
    return g_fail ? 1 : 0;
}
