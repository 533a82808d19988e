// Host preparation of medium volumes (see olx_medium.h).  Plain C++17: no HIP, no context, no environment.
#include "olx_medium.h"
#include <algorithm>
#include <cmath>
namespace olxmed {
GridFault check_grid(const olx_grid& g) {
    for (int a = 0; a < 3; ++a) {
        if (g.n[a] < 1) return GRID_SIZE;
        if (!(g.spacing[a] > 0) || !std::isfinite(g.spacing[a]) || !std::isfinite(g.origin[a])) return GRID_SPACING;
    }
    return GRID_OK;
}
template <Rule R, bool FINITE> static size_t first_bad_of(const float* v, size_t n) {      // (the rule chosen inside the loop halves the speed of a 256^3 check)
    for (size_t o = 0; o < n; ++o)
        if (!(R == POSITIVE ? v[o] > 0.f : v[o] >= 0.f) || (FINITE && !std::isfinite(v[o]))) return o;
    return n;
}
size_t first_bad(const float* v, size_t n, Rule rule, bool finite) {
    if (!v) return n;
    if (rule == POSITIVE) return finite ? first_bad_of<POSITIVE, true>(v, n) : first_bad_of<POSITIVE, false>(v, n);
    return finite ? first_bad_of<NON_NEGATIVE, true>(v, n) : first_bad_of<NON_NEGATIVE, false>(v, n);
}
int first_bad_volume(const size_t* bad, int m, size_t n) {
    const size_t* w = std::min_element(bad, bad + m);      // (the first of equal minima)
    return *w < n ? (int)(w - bad) : -1;
}
template <bool S, bool A, class F> static Planes scan_planes_of(const float* sound_speed, double c_ref, const float* attenuation, int nx, int ny, int nz, F held) {      // (S, A: which volumes exist -- asked per voxel it costs a 256^3 scan a tenth of its speed; held(k) runs as soon as plane k is found held)
    Planes P{std::vector<int>(nz, -1), {}};
    for (int k = 0; k < nz; ++k) {
        bool any = false;
        for (size_t ij = 0; ij < (size_t)nx * ny && !any; ++ij)
            any = (S && (double)sound_speed[ij * nz + k] != c_ref) || (A && attenuation[ij * nz + k] != 0.f);
        if (any) { P.plane_of_k[k] = (int)P.plane_k.size(); P.plane_k.push_back(k); held(k); }
    }
    return P;
}
Planes scan_planes(const float* sound_speed, double c_ref, const float* attenuation, int nx, int ny, int nz) {
    const auto none = [](int) {};
    if (sound_speed) return attenuation ? scan_planes_of<true, true>(sound_speed, c_ref, attenuation, nx, ny, nz, none) : scan_planes_of<true, false>(sound_speed, c_ref, attenuation, nx, ny, nz, none);
    return attenuation ? scan_planes_of<false, true>(sound_speed, c_ref, attenuation, nx, ny, nz, none) : scan_planes_of<false, false>(sound_speed, c_ref, attenuation, nx, ny, nz, none);
}
Planes scan_planes_columns(const float* sound_speed, double c_ref, const float* attenuation, double fpow, int nx, int ny, int nz, std::vector<double>& col) {
    if (sound_speed) return scan_planes_of<true, false>(sound_speed, c_ref, nullptr, nx, ny, nz, [&](int k) { for (size_t ij = 0; ij < (size_t)nx * ny; ++ij) col.push_back(c_ref / (double)sound_speed[ij * nz + k] - 1.0); });
    if (attenuation) return scan_planes_of<false, true>(nullptr, c_ref, attenuation, nx, ny, nz, [&](int k) { for (size_t ij = 0; ij < (size_t)nx * ny; ++ij) col.push_back(np_per_m((double)attenuation[ij * nz + k], fpow)); });
    return scan_planes(nullptr, c_ref, nullptr, nx, ny, nz);
}
Bounds element_plane_bounds(const double* ez, int n, double oz, double hz, int nz) {
    Bounds B{std::vector<int>(n), std::vector<int>(n)};
    for (int e = 0; e < n; ++e) {
        int kf = 0;
        while (kf < nz && !(oz + kf * hz > ez[e])) ++kf;
        int kl = nz - 1;
        while (kl >= 0 && !(oz + kl * hz < ez[e])) --kl;
        B.kfirst[e] = kf; B.klast[e] = kl;
    }
    return B;
}
template <class T, class F> static std::vector<T> per_plane_voxel(size_t nxy, int nz, const std::vector<int>& plane_k, size_t each, F value) {      // `each` values per voxel of the held planes, [plane][ij], a plane at a time: the writes run on end
    std::vector<T> out(plane_k.size() * nxy * each);
    for (size_t p = 0; p < plane_k.size(); ++p)
        for (size_t ij = 0; ij < nxy; ++ij) value(&out[(p * nxy + ij) * each], ij * nz + plane_k[p]);
    return out;
}
std::vector<double> plane_sigma(const float* sound_speed, double c_ref, size_t nxy, int nz, const std::vector<int>& plane_k) {
    return per_plane_voxel<double>(nxy, nz, plane_k, 1, [&](double* out, size_t o) { *out = c_ref / (double)sound_speed[o] - 1.0; });
}
std::vector<float> plane_att(const float* attenuation, double afac, size_t nxy, int nz, const std::vector<int>& plane_k) {
    return per_plane_voxel<float>(nxy, nz, plane_k, 1, [&](float* out, size_t o) { *out = (float)((double)attenuation[o] * afac); });
}
std::vector<float> plane_cells(const float* sound_speed, double c_ref, const float* attenuation, double afac, size_t nxy, int nz, const std::vector<int>& plane_k) {
    return per_plane_voxel<float>(nxy, nz, plane_k, 2, [&](float* out, size_t o) {
        out[0] = sound_speed ? (float)(c_ref / (double)sound_speed[o] - 1.0) : 0.f;
        out[1] = attenuation ? (float)((double)attenuation[o] * afac) : 0.f;
    });
}
std::vector<float> layer_cells(const float* sound_speed, double c_ref, const float* attenuation, double afac, size_t nxy, int nz, const std::vector<int>& layer_lo, const std::vector<int>& layer_hi) {
    std::vector<float> cell(layer_lo.size() * nxy * 2);
    for (size_t g = 0; g < layer_lo.size(); ++g)
        for (size_t ij = 0; ij < nxy; ++ij) {
            double s = 0.0, a = 0.0;      // (fp64 sums from 0 in ascending k, rounded once)
            for (int k = layer_lo[g]; k <= layer_hi[g]; ++k) {
                if (sound_speed) s += c_ref / (double)sound_speed[ij * nz + k] - 1.0;
                if (attenuation) a += (double)attenuation[ij * nz + k] * afac;
            }
            cell[(g * nxy + ij) * 2] = (float)s; cell[(g * nxy + ij) * 2 + 1] = (float)a;
        }
    return cell;
}
std::vector<float> gather_stencil(const std::vector<float>& cell, int planes, int nx, int ny) {
    std::vector<float> tex((size_t)std::max(planes, 1) * nx * ny * 8, 0.f);
    for (int p = 0; p < planes; ++p)
        for (int i = 0; i < nx; ++i)
            for (int j = 0; j < ny; ++j) {
                const int i1 = std::min(i + 1, nx - 1), j1 = std::min(j + 1, ny - 1);
                const int cs[4][2] = {{i, j}, {i, j1}, {i1, j}, {i1, j1}};
                for (int q = 0; q < 4; ++q)
                    for (int t = 0; t < 2; ++t) tex[((((size_t)p * nx + i) * ny + j) * 4 + q) * 2 + t] = cell[(((size_t)p * nx + cs[q][0]) * ny + cs[q][1]) * 2 + t];
            }
    return tex;
}
void layer_runs(const std::vector<int>& plane_k, int G, std::vector<int>& layer_lo, std::vector<int>& layer_hi) {
    int run = 0;
    for (size_t q = 0; q < plane_k.size(); ++q) {
        const bool contiguous = q > 0 && plane_k[q] == plane_k[q - 1] + 1;
        if (!contiguous || run == G) { layer_lo.push_back(plane_k[q]); layer_hi.push_back(plane_k[q]); run = 1; }
        else { layer_hi.back() = plane_k[q]; ++run; }
    }
}
OneLine detect_one_line(const std::vector<float>& med, size_t cells) {
    OneLine L{true, 0.0, 0.0};
    for (size_t q = 0; q < cells && L.one; ++q) {
        const double sg = med[q * 8], ab = med[q * 8 + 1];
        if (sg == 0.0 && ab == 0.0) continue;
        if (L.s_ref == 0.0 && L.a_ref == 0.0) { L.s_ref = sg; L.a_ref = ab; if (L.s_ref == 0.0) L.one = false; continue; }
        if (sg * L.a_ref != ab * L.s_ref) L.one = false;
    }
    return L;
}
std::vector<float> impedance_volume(const float* density, double rho0, const float* sound_speed, double c0, size_t off, size_t count) {
    std::vector<float> iz(count);
    for (size_t o = 0; o < count; ++o)
        iz[o] = (float)(1e-4 / (2.0 * (density ? (double)density[off + o] : rho0) * (sound_speed ? (double)sound_speed[off + o] : c0)));
    return iz;
}
}  // namespace olxmed
