// C entry points into kernel 2's host planning (openlifu-python_amd/csrc/olx_plan.cpp) for the CPU tests of the parity matrices
// (tests/test_gpu_lattice_matrix.py builds it with  g++ -std=c++17 -O1 -shared -fPIC tools/plan_query.cpp openlifu-python_amd/csrc/olx_plan.cpp,
// and a second time with -DOLX_DEV_PINS for the developer rows): the decision itself -- olq_variant returns the variant string of the real
// decide_variant, which every row of the lattice, 2a / 2b / 2c and heterogeneous tables is compared with -- and the quantities the lattice matrix's
// independent restatement of the rule (plan_rule) takes from the real code instead of restating them: detect_lattice (with the clamp bound over real
// and virtual lattice points), coset_tiles16, pack_columns, toep_plan and fp8_first_plane.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../openlifu-python_amd/csrc/olx_plan.h"

using namespace olxplan;

extern "C" {

// out = {ok, ax, ay, mx, my, nsa, nsb, clamp}; pos = [3][n] (SoA) [m]; lo / hi = bounding box of the planned slab [m]
void olq_lattice(int n, const double* pos, const double* spacing, const double* lo, const double* hi, double dmin, int* out) {
    Lattice L;
    detect_lattice(L, true, n, pos, spacing, lo, hi, dmin);
    const int v[8] = {L.ok ? 1 : 0, L.ax, L.ay, L.mx, L.my, L.nsa, L.nsb, L.clamp ? 1 : 0};
    std::copy(v, v + 8, out);
}

long long olq_coset_tiles16(int wx, int wy, int mx, int my, int nt) { return coset_tiles16(wx, wy, mx, my, nt); }

// column packing of F foci x n_img mirror images into tiles of <= maxc columns: returns the tile count, sizes[t] = columns of tile t (t < max_tiles),
// *max_targets = the most store targets any column carries
int olq_pack(int n, int F, int fold_x, int fold_y, const int* px, const int* py, const double* delays, const double* apod, const double* area, double freq,
             int maxc, int* sizes, int max_tiles, int* max_targets) {
    const int n_img = (fold_x ? 2 : 1) * (fold_y ? 2 : 1);
    const std::vector<int> perm = mirror_perms(n, n_img, fold_x != 0, fold_y != 0, px, py, 4);
    Steering S;
    S.n = n; S.F = F; S.n_img = n_img; S.perm = perm.data(); S.delays = delays; S.apod = apod; S.area = area; S.freq = freq;
    const Tiles tiles = pack_columns(S, maxc);
    *max_targets = 0;
    for (size_t t = 0; t < tiles.size(); ++t) {
        if ((int)t < max_tiles) sizes[t] = (int)tiles[t].size();
        for (const Col& c : tiles[t]) *max_targets = std::max(*max_targets, c.ntgt);
    }
    return (int)tiles.size();
}

// kernel 2f's row tiles per block (NM); *kyw = y positions per block
int olq_toep_nm(int ax, int mx, int my, int xs, int wx, int wy, int nz, int dir_lattice, int* kyw) {
    const ToepPlan T = toep_plan(ax, mx, my, xs, wx, wy, nz, dir_lattice != 0);
    *kyw = T.kyw;
    return T.nm;
}

// the e4m3 rule: first plane of the e4m3 products (0 = every plane, -1 = refused) for known foci [F][3]; -2 = the array is no lattice on this grid
int olq_fp8_first_plane(int n, const double* pos, const double* area, const double* apod, int F, const double* foci, const double* origin,
                        const double* spacing, const int* gn, int x_begin, int x_count) {
    double lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
        const int b = a == 0 ? x_begin : 0, cnt = a == 0 ? x_count : gn[a];
        lo[a] = origin[a] + b * spacing[a]; hi[a] = origin[a] + (b + cnt - 1) * spacing[a];
    }
    Lattice L;
    detect_lattice(L, true, n, pos, spacing, lo, hi, 0.5 * std::min({spacing[0], spacing[1], spacing[2]}));
    if (!L.ok) return -2;
    std::vector<double> cache;
    return fp8_first_plane(n, pos, area, apod, F, foci, origin, spacing, gn, x_begin, x_count, L, cache);
}

int olq_fp8_split_pays(int x_count, int ny, int nz, int F, int cut) { return fp8_split_pays(x_count, ny, nz, F, cut) ? 1 : 0; }

// The real decision (decide_variant) for a plan described by plain values; olq_variant returns the length of its variant string, the string itself in out (cap bytes).
//   pos = [3][n] (SoA) [m], area = [n], delays / apod = [F][n], foci = [F][3] [m] or null (not known), flags = the plan flags of include/olx.h
//   mods = {the elements are flat, axis-aligned and of equal size (what lets the per-term factors into the lattice tables), intensity stored (OLX_INTENSITY_STORED)},
//   elem = {width, length of element 0 [m], uniform absorption [Np/m]}, family_pin / fp8_pin = OLX_FIELD_VARIANT / OLX_FP8_CORRECTION or null,
//   medium = null (homogeneous) or {marched, one-sum, non-trivial planes, layers, planes per layer} as olx_field_set_medium established them.
// What olx_field_plan derives from these before it asks for the decision -- flatness, the clamp and near classes, the lattice, the mirror folds, the family
// pin's kind -- is derived here in the same way; a build with -DOLX_DEV_PINS honours the forcing value of fp8_pin as the developer library does.
static VariantPlan plan_of(int n, const double* pos, const double* area, int F, const double* delays, const double* apod, const double* foci, const double* origin,
                           const double* spacing, const int* gn, int x_begin, int x_count, double freq, double c, double rho, double p0_pa, unsigned flags, const int* mods,
                           const double* elem, const char* family_pin, const char* fp8_pin, const int* medium) {
    constexpr unsigned DIRECTIVITY = 16u;      // OLX_FIELD_DIRECTIVITY
    VariantIn in;
    in.n = n; in.F = F; in.pos = pos; in.area = area; in.delays = delays; in.apod = apod; in.foci = foci;
    in.freq = freq; in.c = c; in.p0_pa = p0_pa; in.x_begin = x_begin; in.x_count = x_count; in.flags = flags;
    for (int a = 0; a < 3; ++a) { in.origin[a] = origin[a]; in.spacing[a] = spacing[a]; in.gn[a] = gn[a]; }
    in.directivity = (flags & DIRECTIVITY) != 0; in.absorb_np_m = elem[2]; in.size0 = elem[0]; in.size1 = elem[1];
    const double rev = freq / c, dmin = 0.5 * std::min({spacing[0], spacing[1], spacing[2]});
    const double* ez = pos + 2 * (size_t)n;
    in.flat = std::all_of(ez, ez + n, [&](double z) { return z == ez[0]; });
    olx::FieldParams& P = in.fp;
    P.nx = x_count; P.ny = gn[1]; P.nz = gn[2]; P.n_el = n; P.x_begin = x_begin;
    P.hx = (float)(spacing[0] * rev); P.hy = (float)(spacing[1] * rev); P.hz = (float)(spacing[2] * rev);
    P.dmin2 = (float)(dmin * dmin * rev * rev); P.inten_scale = (float)(1e-4 / (2.0 * rho * c));
    P.flat_ez = (float)((ez[0] - origin[2]) * rev);
    { const double kz = std::rint((ez[0] - origin[2]) / spacing[2]); P.flat_kz = (float)kz; P.flat_fz = (float)(((ez[0] - origin[2]) - kz * spacing[2]) * rev); }
    P.absorb_l2 = (float)(in.absorb_np_m * (c / freq) * 1.4426950408889634);
    P.vox = (long long)x_count * gn[1] * gn[2];
    P.flags = ((flags & 7u) | FLAG_OUT_PMAG) & ~(((flags & FLAG_OUT_INTENSITY) && !mods[1]) ? FLAG_OUT_INTENSITY : 0u);
    double lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
        const int b = a == 0 ? x_begin : 0, cnt = a == 0 ? x_count : gn[a];
        lo[a] = origin[a] + b * spacing[a]; hi[a] = origin[a] + (b + cnt - 1) * spacing[a];
    }
    double min_d2 = 1e300;
    for (int e = 0; e < n; ++e) {
        double d2 = 0;
        for (int a = 0; a < 3; ++a) {
            const double p = pos[(size_t)a * n + e], d = p < lo[a] ? lo[a] - p : (p > hi[a] ? p - hi[a] : 0.0);
            d2 += d * d;
        }
        min_d2 = std::min(min_d2, d2);
    }
    in.clamp = min_d2 < 4.0 * dmin * dmin;
    in.min_dist = in.clamp ? dmin : std::sqrt(min_d2);
    in.near = in.clamp || in.min_dist < 0.25 * c / freq;
    Lattice L;
    detect_lattice(L, in.flat, n, pos, spacing, lo, hi, dmin);
    in.lat = &L;
    in.force_kind = !family_pin ? 0 : !strcmp(family_pin, "general") ? 1 : !strcmp(family_pin, "shared") ? 2 : !strcmp(family_pin, "mfma") ? 3
                    : (!strcmp(family_pin, "lattice") || !strcmp(family_pin, "lattice2d")) ? 4 : 0;
    in.dir_lattice = in.modifier() && !(flags & FLAG_OUT_COMPLEX) && in.flat && (!in.directivity || mods[0]);
    in.allow_shared = in.force_kind != 1 && (!in.modifier() || in.dir_lattice);
    // the element set symmetric about the grid's centre plane of an axis (1e-12 m)
    auto mirror = [&](int axis, std::vector<int>& perm) {
        const double ctr = origin[axis] + 0.5 * (gn[axis] - 1) * spacing[axis];
        perm.assign(n, -1);
        std::vector<char> used(n, 0);
        for (int e = 0; e < n; ++e) {
            int hit = -1;
            for (int o = 0; o < n && hit < 0; ++o) {
                if (used[o] || std::fabs(pos[(size_t)axis * n + o] - (2.0 * ctr - pos[(size_t)axis * n + e])) > 1e-12) continue;
                bool same = true;
                for (int a = 0; a < 3; ++a) if (a != axis && std::fabs(pos[(size_t)a * n + o] - pos[(size_t)a * n + e]) > 1e-12) same = false;
                if (same) hit = o;
            }
            if (hit < 0) return false;
            used[hit] = 1; perm[e] = hit;
        }
        return true;
    };
    std::vector<int> px, py;
    in.mx = (in.allow_shared && x_begin == 0 && x_count == gn[0] && gn[0] >= 2 && n <= 8192 && mirror(0, px)) ? 2 : 1;
    in.my = (in.allow_shared && gn[1] >= 2 && n <= 8192 && mirror(1, py)) ? 2 : 1;
    in.px = px.data(); in.py = py.data();
    if (medium) { in.hetero = true; in.marched = medium[0] != 0; in.march_one = medium[1] != 0; in.n_planes = medium[2]; in.n_layers = medium[3]; in.planes_per_layer = medium[4]; }
    if (family_pin) in.pins.family = !strcmp(family_pin, "lattice") ? FamilyPin::lattice : !strcmp(family_pin, "lattice2d") ? FamilyPin::lattice2d : FamilyPin::other;
    if (fp8_pin && !strcmp(fp8_pin, "0")) in.pins.fp8 = -1;
#ifdef OLX_DEV_PINS
    if (fp8_pin && strcmp(fp8_pin, "0") != 0) in.pins.fp8 = 1;
#endif
    std::vector<double> inferred;      // (external delays: geometric?  As configure_variant resolves them)
    if (!in.foci && !in.hetero && variant_reads_foci(in) && infer_foci(in.flat, n, F, pos, delays, c, origin[2] + 0.5 * (gn[2] - 1) * spacing[2], inferred)) in.foci = inferred.data();
    std::vector<double> nf_s2;
    int slot_rows = L.nsbp;
    return decide_variant(in, nf_s2, slot_rows);
}

int olq_variant(int n, const double* pos, const double* area, int F, const double* delays, const double* apod, const double* foci, const double* origin,
                const double* spacing, const int* gn, int x_begin, int x_count, double freq, double c, double rho, double p0_pa, unsigned flags, const int* mods,
                const double* elem, const char* family_pin, const char* fp8_pin, const int* medium, char* out, int cap) {
    const VariantPlan p = plan_of(n, pos, area, F, delays, apod, foci, origin, spacing, gn, x_begin, x_count, freq, c, rho, p0_pa, flags, mods, elem, family_pin, fp8_pin, medium);
    snprintf(out, (size_t)cap, "%s", p.variant.c_str());
    return (int)p.variant.size();
}

// The block records of the same plan as the launches read them (build_variant_blocks: kernel 2g's position sets heaviest first): 8 ints per record
// {ibase, jbase, k0, npos, KY, ky_magic, KX, 0} into rec (cap records), *n_near = the records of the launch below the e4m3 cut (they come last; each
// side is a launch of its own, ids from 0), *is_2g = the plan launches kernel 2g.  Returns the record count, 0 for a plan without coset records, -1 when
// the records are refused.
int olq_blocks(int n, const double* pos, const double* area, int F, const double* delays, const double* apod, const double* foci, const double* origin,
               const double* spacing, const int* gn, int x_begin, int x_count, double freq, double c, double rho, double p0_pa, unsigned flags, const int* mods,
               const double* elem, const char* family_pin, const char* fp8_pin, const int* medium, int* rec, int cap, int* n_near, int* is_2g) {
    const VariantPlan p = plan_of(n, pos, area, F, delays, apod, foci, origin, spacing, gn, x_begin, x_count, freq, c, rho, p0_pa, flags, mods, elem, family_pin, fp8_pin, medium);
    *n_near = (int)p.blocks_near; *is_2g = p.use_cosetp ? 1 : 0;
    if (!p.use_coset) return 0;
    std::vector<olx::CosetBlock> blk;
    std::string why;
    if (!build_variant_blocks(p, blk, why)) return -1;
    static_assert(sizeof(olx::CosetBlock) == 8 * sizeof(int), "eight ints per record");
    if ((int)blk.size() <= cap) memcpy(rec, blk.data(), blk.size() * sizeof(olx::CosetBlock));
    return (int)blk.size();
}

}  // extern "C"
