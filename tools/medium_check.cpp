// CPU-side checker of the medium preparation (openlifu-python_amd/csrc/olx_medium.cpp), built by tests/test_medium_prep_host.py with
// g++ -fsanitize=address,undefined and run without a GPU:  medium_check [random cases = 300] [seed = 147]
// Every output of the unit is compared BIT FOR BIT with a restatement written here from the definitions (sections 5.9, 5.10,
// 5.12, 5.13 for the compact columns): one voxel at a time through at(), whole-range scans without early exits, no helper of the unit.
// A mismatch prints "FAIL <rule>: ..." and the program exits 1.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "../openlifu-python_amd/csrc/olx_medium.h"

using namespace olxmed;

static int g_fail = 0, g_cases = 0;
#define FAIL(rule, ...) do { ++g_fail; fprintf(stderr, "FAIL %s: ", rule); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); if (g_fail > 20) exit(1); } while (0)
template <class T> static void same(const char* rule, const std::string& name, const char* what, const std::vector<T>& got, const std::vector<T>& want) {
    if (got.size() != want.size()) { FAIL(rule, "%s: %s has %zu entries, expected %zu", name.c_str(), what, got.size(), want.size()); return; }
    for (size_t q = 0; q < got.size(); ++q)
        if (memcmp(&got[q], &want[q], sizeof(T))) { FAIL(rule, "%s: %s[%zu] = %.17g, expected %.17g", name.c_str(), what, q, (double)got[q], (double)want[q]); return; }
}

struct Case {
    std::string name;
    int nx, ny, nz;
    std::vector<float> ss, att, rho;     // empty = null
    double c_ref = 1500.0, freq = 400e3, power = 0.9, oz = 5e-3, hz = 0.5e-3, rho0 = 1000.0;
    int G = 3;
    std::vector<double> ez;
    Case(const std::string& name_, int nx_, int ny_, int nz_) : name(name_), nx(nx_), ny(ny_), nz(nz_) {}
    const float* p(const std::vector<float>& v) const { return v.empty() ? nullptr : v.data(); }
    float at(const std::vector<float>& v, int i, int j, int k) const { return v[((size_t)i * ny + j) * nz + k]; }
};

// ---- the restatement, one voxel at a time ------------------------------------------------------------------------------------------------
static double r_sigma(const Case& c, int i, int j, int k) { return c.c_ref / (double)c.at(c.ss, i, j, k) - 1.0; }
static bool r_held(const Case& c, int k) {
    int hits = 0;
    for (int i = 0; i < c.nx; ++i)
        for (int j = 0; j < c.ny; ++j) {
            if (!c.ss.empty() && (double)c.at(c.ss, i, j, k) != c.c_ref) ++hits;
            if (!c.att.empty() && c.at(c.att, i, j, k) != 0.f) ++hits;
        }
    return hits > 0;
}
// texels of planes (summed = false, lo = hi) or of layers [lo, hi] of planes (fp64 sums from 0, rounded once): slot q of cell (i, j) is voxel
// (i + (q >> 1), j + (q & 1)) pulled back inside the grid
static std::vector<float> r_texels(const Case& c, const std::vector<int>& lo, const std::vector<int>& hi, double afac, bool summed) {
    std::vector<float> t((lo.empty() ? 1 : lo.size()) * (size_t)c.nx * c.ny * 8, 0.f);
    for (size_t p = 0; p < lo.size(); ++p)
        for (int i = 0; i < c.nx; ++i)
            for (int j = 0; j < c.ny; ++j)
                for (int q = 0; q < 4; ++q) {
                    int ii = i + (q >> 1), jj = j + (q & 1);
                    if (ii > c.nx - 1) ii = c.nx - 1;
                    if (jj > c.ny - 1) jj = c.ny - 1;
                    double s = 0, a = 0;
                    for (int k = lo[p]; k <= hi[p]; ++k) {
                        if (!c.ss.empty()) s += r_sigma(c, ii, jj, k);
                        if (!c.att.empty()) a += (double)c.at(c.att, ii, jj, k) * afac;
                    }
                    float* o = &t[(((p * c.nx + i) * c.ny + j) * 4 + q) * 2];
                    o[0] = (float)s; o[1] = (float)a;
                    if (!summed && !c.ss.empty()) o[0] = (float)r_sigma(c, ii, jj, lo[p]);
                    if (!summed && !c.att.empty()) o[1] = (float)((double)c.at(c.att, ii, jj, lo[p]) * afac);      // (keeps the sign of a -0.0f)
                }
    return t;
}
static int r_bad_rule(float v, Rule rule, bool finite) { return std::isnan(v) || (rule == POSITIVE ? v <= 0.f : v < 0.f) || (finite && std::isinf(v)); }
static size_t r_first_bad(const std::vector<float>& v, Rule rule, bool finite) {
    size_t first = v.size();
    for (size_t o = v.size(); o-- > 0;)
        if (r_bad_rule(v[o], rule, finite)) first = o;
    return first;
}

static void run(const Case& c) {
    ++g_cases;
    const int nx = c.nx, ny = c.ny, nz = c.nz;
    const size_t nxy = (size_t)nx * ny;
    const double fpow = std::pow(c.freq * 1e-6, c.power), lambda = c.c_ref / c.freq;
    const double a_m = fpow * 100.0 / 8.685889638065035, a_w = fpow * 100.0 * (1.0 / 8.685889638065035) * lambda;
    same<double>("attenuation factors", c.name, "Np/m, Np per wavelength", {np_per_m_factor(c.freq, c.power), np_per_wavelength_factor(c.freq, c.power, lambda)}, {a_m, a_w});
    // planes
    const Planes pl = scan_planes(c.p(c.ss), c.c_ref, c.p(c.att), nx, ny, nz);
    std::vector<int> of_k(nz, -1), ks;
    for (int k = 0; k < nz; ++k)
        if (r_held(c, k)) { of_k[k] = (int)ks.size(); ks.push_back(k); }
    same("plane rule", c.name, "plane_of_k", pl.plane_of_k, of_k);
    same("plane rule", c.name, "plane_k", pl.plane_k, ks);
    // stencil of the planes, with both factors (2h / 2m and 4h)
    for (double afac : {a_w, a_m * lambda})
        same("stencil gather", c.name, "plane texels", gather_stencil(plane_cells(c.p(c.ss), c.c_ref, c.p(c.att), afac, nxy, nz, ks), (int)ks.size(), nx, ny),
             r_texels(c, ks, ks, afac, false));
    // layers: a held plane opens a layer unless the plane below is held and the open layer has fewer than G planes
    std::vector<int> lo, hi, rlo, rhi;
    for (int k = 0, open = 0; k < nz; ++k) {
        if (of_k[k] < 0) { open = 0; continue; }
        if (open == 0 || open == c.G) { rlo.push_back(k); rhi.push_back(k); open = 1; }
        else { rhi.back() = k; ++open; }
    }
    layer_runs(ks, c.G, lo, hi);
    same("layering", c.name, "layer_lo", lo, rlo);
    same("layering", c.name, "layer_hi", hi, rhi);
    same("layer sum", c.name, "layer texels", gather_stencil(layer_cells(c.p(c.ss), c.c_ref, c.p(c.att), a_w, nxy, nz, rlo, rhi), (int)rlo.size(), nx, ny),
         r_texels(c, rlo, rhi, a_w, true));
    // one-line detection on the plane texels' own values
    {
        const std::vector<float> med = r_texels(c, ks, ks, a_w, false);
        OneLine R{true, 0.0, 0.0};
        bool have = false;
        for (size_t q = 0; q < ks.size() * nxy; ++q) {
            const double s = med[q * 8], a = med[q * 8 + 1];
            if (s == 0.0 && a == 0.0) continue;
            if (!have) { have = true; R.s_ref = s; R.a_ref = a; }
            if (R.s_ref == 0.0 || s * R.a_ref != a * R.s_ref) R.one = false;
        }
        const OneLine L = detect_one_line(med, ks.size() * nxy);
        if (L.one != R.one || memcmp(&L.s_ref, &R.s_ref, 8) || memcmp(&L.a_ref, &R.a_ref, 8))
            FAIL("one-line detection", "%s: (%d, %.9g, %.9g), expected (%d, %.9g, %.9g)", c.name.c_str(), L.one, L.s_ref, L.a_ref, R.one, R.s_ref, R.a_ref);
    }
    // compact columns
    std::vector<double> sg;
    std::vector<float> af;
    for (int k : ks)
        for (int i = 0; i < nx; ++i)
            for (int j = 0; j < ny; ++j) {
                if (!c.ss.empty()) sg.push_back(r_sigma(c, i, j, k));
                if (!c.att.empty()) af.push_back((float)((double)c.at(c.att, i, j, k) * a_m));
            }
    if (!c.ss.empty()) same("compact columns", c.name, "sigma", plane_sigma(c.p(c.ss), c.c_ref, nxy, nz, ks), sg);
    // kernels 1m / 1a: the planes of one volume alone and their columns, found in one pass
    for (int a = 0; a < 2; ++a) {
        const std::vector<float>& v = a ? c.att : c.ss;
        std::vector<int> of1(nz, -1), k1;
        std::vector<double> want, got;
        for (int k = 0; k < nz; ++k) {
            bool held = false;
            for (int i = 0; i < nx; ++i)
                for (int j = 0; j < ny; ++j)
                    if (!v.empty() && (a ? c.at(v, i, j, k) != 0.f : (double)c.at(v, i, j, k) != c.c_ref)) held = true;
            if (!held) continue;
            of1[k] = (int)k1.size(); k1.push_back(k);
            for (int i = 0; i < nx; ++i)
                for (int j = 0; j < ny; ++j) want.push_back(a ? (double)c.at(v, i, j, k) * fpow * 100.0 / 8.685889638065035 : c.c_ref / (double)c.at(v, i, j, k) - 1.0);
        }
        const Planes p1 = scan_planes_columns(a ? nullptr : c.p(c.ss), c.c_ref, a ? c.p(c.att) : nullptr, fpow, nx, ny, nz, got);
        same("plane rule", c.name, a ? "plane_of_k of the attenuation alone" : "plane_of_k of the sound speed alone", p1.plane_of_k, of1);
        same("plane rule", c.name, a ? "plane_k of the attenuation alone" : "plane_k of the sound speed alone", p1.plane_k, k1);
        same("compact columns", c.name, a ? "a [Np/m] fp64" : "sigma in one pass", got, want);
    }
    if (!c.att.empty()) same("compact columns", c.name, "a [Np/m] float", plane_att(c.p(c.att), a_m, nxy, nz, ks), af);
    // element plane bounds: first plane strictly above, last plane strictly below
    std::vector<int> rkf, rkl;
    for (double ez : c.ez) {
        int f = nz, l = -1;
        for (int k = nz - 1; k >= 0; --k) if (c.oz + k * c.hz > ez) f = k;
        for (int k = 0; k < nz; ++k) if (c.oz + k * c.hz < ez) l = k;
        rkf.push_back(f); rkl.push_back(l);
    }
    const Bounds B = element_plane_bounds(c.ez.data(), (int)c.ez.size(), c.oz, c.hz, nz);
    same("element bounds", c.name, "kfirst", B.kfirst, rkf);
    same("element bounds", c.name, "klast", B.klast, rkl);
    // impedance: the whole grid and a slab of it
    const size_t x0 = nx / 3, xc = nx - x0 - nx / 4;
    for (auto [off, cnt] : {std::pair<size_t, size_t>{0, nxy * nz}, std::pair<size_t, size_t>{x0 * ny * nz, xc * ny * nz}}) {
        std::vector<float> iz;
        for (size_t o = off; o < off + cnt; ++o)
            iz.push_back((float)(1e-4 / (2.0 * (c.rho.empty() ? c.rho0 : (double)c.rho[o]) * (c.ss.empty() ? c.c_ref : (double)c.ss[o]))));
        same("impedance", c.name, "1e-4 / (2 rho c)", impedance_volume(c.p(c.rho), c.rho0, c.p(c.ss), c.c_ref, off, cnt), iz);
    }
}

// ---- volumes -----------------------------------------------------------------------------------------------------------------------------
static std::mt19937 g_rng;
static double uni() { return std::uniform_real_distribution<double>(0.0, 1.0)(g_rng); }
// materials: 0 water (the reference), 1 bone, 2 a lossy soft inclusion SLOWER than the reference, 3 lossless and slower
static void paint(Case& c, int materials, double fill, bool with_ss, bool with_att, bool with_rho) {
    const size_t n = (size_t)c.nx * c.ny * c.nz;
    if (with_ss) c.ss.assign(n, (float)c.c_ref);
    if (with_att) c.att.assign(n, 0.f);
    if (with_rho) c.rho.assign(n, 1000.f);
    std::vector<char> plane(c.nz);
    for (auto& p : plane) p = uni() < fill;
    for (int i = 0; i < c.nx; ++i)
        for (int j = 0; j < c.ny; ++j)
            for (int k = 0; k < c.nz; ++k) {
                if (!plane[k] || uni() < 0.3) continue;
                const int m = 1 + (int)(uni() * (materials - 1));
                const size_t o = ((size_t)i * c.ny + j) * c.nz + k;
                const double wob = materials > 2 ? 1.0 + 0.04 * uni() : 1.0;
                if (with_ss) c.ss[o] = (float)((m == 1 ? 2800.0 : m == 2 ? 1450.0 : 1480.0) * wob);
                if (with_att) c.att[o] = (float)((m == 1 ? 8.0 : m == 2 ? 0.6 : 0.0) * wob);
                if (with_rho) c.rho[o] = m == 1 ? 1900.f : 1050.f;
            }
}
static void elements(Case& c) {
    c.ez = {c.oz - 1e-3, c.oz + c.nz * c.hz + 1e-3, c.oz, c.oz + (c.nz / 2) * c.hz, c.oz + (c.nz - 1) * c.hz, -1e-3, 0.0};
    for (int q = 0; q < 6; ++q) c.ez.push_back(c.oz + (uni() * (c.nz + 2) - 1) * c.hz);
}

static void expect(bool ok, const char* rule, const char* what) { if (!ok) FAIL(rule, "%s", what); }

static void fixed_cases() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // volume checks: NaN, +-inf, 0 and a negative value at the first, middle and last voxel
    for (float bad : {nan, inf, -inf, 0.f, -0.f, -1.f})
        for (size_t n : {1u, 2u, 9u})
            for (size_t at : {(size_t)0, n / 2, n - 1})
                for (Rule rule : {POSITIVE, NON_NEGATIVE})
                    for (bool finite : {true, false}) {
                        std::vector<float> v(n, 1.f);
                        v[at] = bad;
                        if (at + 1 < n && uni() < 0.5) v[n - 1] = nan;      // (a later offender does not win)
                        ++g_cases;
                        if (first_bad(v.data(), n, rule, finite) != r_first_bad(v, rule, finite))
                            FAIL("volume check", "value %g at %zu of %zu, rule %d, finite %d: %zu", (double)bad, at, n, (int)rule, (int)finite, first_bad(v.data(), n, rule, finite));
                    }
    expect(first_bad(nullptr, 0, POSITIVE) == 0, "volume check", "an empty volume has no offender");
    // kernel 2ph's order: voxel by voxel, sound speed, attenuation, density
    for (int trial = 0; trial < 60; ++trial) {
        const size_t n = 1 + (size_t)(uni() * 7);
        std::vector<float> v[3] = {std::vector<float>(n, 1500.f), std::vector<float>(n, 0.f), std::vector<float>(n, 1000.f)};
        bool given[3];
        for (int q = 0; q < 3; ++q) { given[q] = uni() < 0.8; if (uni() < 0.6) v[q][(size_t)(uni() * n)] = q == 1 ? -1.f : 0.f; }
        int want = -1;
        for (size_t o = 0; o < n && want < 0; ++o)
            for (int q = 0; q < 3 && want < 0; ++q)
                if (given[q] && r_bad_rule(v[q][o], q == 1 ? NON_NEGATIVE : POSITIVE, true)) want = q;
        size_t bad[3];
        for (int q = 0; q < 3; ++q) bad[q] = given[q] ? first_bad(v[q].data(), n, q == 1 ? NON_NEGATIVE : POSITIVE) : n;
        ++g_cases;
        if (first_bad_volume(bad, 3, n) != want) FAIL("interleaved priority", "trial %d: volume %d wins, expected %d", trial, first_bad_volume(bad, 3, n), want);
    }
    // grid check: axis by axis, sizes before spacing
    {
        const double dnan = std::nan(""), dinf = std::numeric_limits<double>::infinity();
        olx_grid g{{0, 0, 0}, {1e-3, 1e-3, 1e-3}, {4, 5, 6}};
        expect(check_grid(g) == GRID_OK, "grid check", "a sane grid");
        for (int a = 0; a < 3; ++a) {
            olx_grid b = g; b.n[a] = 0; expect(check_grid(b) == GRID_SIZE, "grid check", "size 0");
            for (double s : {0.0, -1e-3, dnan, dinf}) { b = g; b.spacing[a] = s; expect(check_grid(b) == GRID_SPACING, "grid check", "bad spacing"); }
            for (double o : {dnan, -dinf}) { b = g; b.origin[a] = o; expect(check_grid(b) == GRID_SPACING, "grid check", "bad origin"); }
        }
        olx_grid b = g; b.spacing[0] = 0; b.n[1] = 0; expect(check_grid(b) == GRID_SPACING, "grid check", "axis 0's spacing comes before axis 1's size");
        b = g; b.n[0] = 0; b.spacing[0] = 0; expect(check_grid(b) == GRID_SIZE, "grid check", "an axis' size comes before its spacing");
        g_cases += 3;
    }
    // the plane rule's comparisons
    {
        Case c{"c_ref a double no float equals", 3, 2, 4};
        c.c_ref = 1500.1; c.ss.assign(24, 1500.1f); elements(c); run(c);      // (float)c_ref == every voxel, (double)voxel != c_ref: all planes held
        expect((int)scan_planes(c.p(c.ss), c.c_ref, nullptr, 3, 2, 4).plane_k.size() == 4, "plane rule", "sound speed compared as double: every plane held");
        c.name = "c_ref equal after the conversion"; c.c_ref = (double)1500.1f; run(c);
        expect(scan_planes(c.p(c.ss), c.c_ref, nullptr, 3, 2, 4).plane_k.empty(), "plane rule", "sound speed equal to c_ref after float -> double: no plane");
        Case z{"attenuation -0.0f", 3, 2, 4};
        z.att.assign(24, -0.f); elements(z); run(z);
        expect(scan_planes(nullptr, 1500.0, z.p(z.att), 3, 2, 4).plane_k.empty(), "plane rule", "-0.0f is no attenuation");
        z.name = "attenuation -0.0f beside a held voxel"; z.att[1 * 4 + 2] = 2.f; run(z);      // (plane 2 is held; its other texels keep -0.0f)
        Case s{"one slower lossless voxel", 4, 3, 5};
        s.ss.assign(60, 1500.f); s.att.assign(60, 0.f); s.ss[(1 * 3 + 2) * 5 + 3] = 1450.f; elements(s); run(s);
    }
    // layering: G = 3 over a run of 7 planes, a gap, a single plane
    {
        Case c{"layering 7 + gap + 1", 3, 4, 14};
        c.att.assign((size_t)3 * 4 * 14, 0.f);
        for (int k : {2, 3, 4, 5, 6, 7, 8, 11}) c.att[(size_t)(k % 12) * 14 + k] = 4.f + k;
        paint(c, 3, 0.0, true, false, true);
        for (int k = 2; k <= 8; ++k) for (size_t ij = 0; ij < 12; ++ij) c.ss[ij * 14 + k] = 2500.f + 7.3f * (float)(ij + k);
        elements(c); run(c);
        std::vector<int> lo, hi;
        layer_runs({2, 3, 4, 5, 6, 7, 8, 11}, 3, lo, hi);
        expect(lo == std::vector<int>{2, 5, 8, 11} && hi == std::vector<int>{4, 7, 8, 11}, "layering", "7 + gap + 1 planes at G = 3 are layers 2-4, 5-7, 8, 11");
    }
    // one-line detection on stored texel values
    {
        auto med = [](std::initializer_list<std::pair<float, float>> cells) { std::vector<float> m; for (auto& t : cells) { m.push_back(t.first); m.push_back(t.second); m.resize(m.size() + 6, 9.f); } return m; };
        OneLine L = detect_one_line(med({{0.f, 0.f}, {-0.25f, 0.5f}, {-0.5f, 1.f}, {0.f, 0.f}}), 4);
        expect(L.one && L.s_ref == -0.25 && L.a_ref == 0.5, "one-line detection", "two proportional materials lie on one line");
        L = detect_one_line(med({{-0.25f, 0.5f}, {-0.5f, 1.f}, {-0.25f, 0.75f}}), 3);
        expect(!L.one, "one-line detection", "a third material off the line");
        L = detect_one_line(med({{0.f, 0.f}, {0.f, 0.5f}, {-0.5f, 1.f}}), 3);
        expect(!L.one && L.s_ref == 0.0 && L.a_ref == 0.5, "one-line detection", "a first texel with sigma = 0 and a' != 0 has no kappa");
        L = detect_one_line(med({{0.f, 0.f}}), 1);
        expect(L.one && L.s_ref == 0.0, "one-line detection", "no texel off the origin: one, but s_ref = 0");
        g_cases += 4;
    }
}

int main(int argc, char** argv) {
    const int cases = argc > 1 ? atoi(argv[1]) : 300;
    g_rng.seed(argc > 2 ? (unsigned)atoi(argv[2]) : 147u);
    fixed_cases();
    const int shapes[][3] = {{1, 5, 4}, {5, 1, 4}, {1, 1, 1}, {4, 3, 1}, {1, 1, 6}, {2, 2, 3}, {7, 5, 9}, {3, 8, 14}, {12, 11, 14}};
    for (int q = 0; q < cases; ++q) {
        const int* s = shapes[q % 9];
        Case c{"case " + std::to_string(q), s[0], s[1], s[2]};
        const int nulls = (q / 9) % 4;                      // both volumes, null attenuation, null sound speed, both null
        const int fill = (q / 36) % 3;                      // some planes, every plane, none
        paint(c, 2 + q % 3, fill == 0 ? 0.5 : fill == 1 ? 1.0 : 0.0, !(nulls & 2), !(nulls & 1), q % 2 == 0);
        c.G = 1 + q % 4; c.power = q % 5 ? 0.9 : 1.3; c.freq = q % 3 ? 400e3 : 1.1e6; c.hz = q % 2 ? 0.5e-3 : 0.3e-3;
        if (fill == 1 && !(nulls & 1))                      // (every plane held for certain)
            for (int k = 0; k < c.nz; ++k) c.att[k] = 3.f;
        elements(c);
        run(c);
    }
    printf("medium_check: %d cases, %d mismatches\n", g_cases, g_fail);
    return g_fail ? 1 : 0;
}
