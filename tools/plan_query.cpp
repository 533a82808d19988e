// C entry points into the lattice kernels' host planning (openlifu-python_amd/csrc/olx_plan.cpp) for the CPU tests of the lattice parity matrix
// (tests/test_gpu_lattice_matrix.py builds it with  g++ -std=c++17 -O1 -shared -fPIC tools/plan_query.cpp openlifu-python_amd/csrc/olx_plan.cpp):
// the quantities the matrix's restated decision rule takes from the real code instead of restating them -- detect_lattice (with the clamp bound over
// real and virtual lattice points), coset_tiles16, pack_columns, toep_plan and fp8_first_plane.  The decision itself (configure_variant, olx.hip)
// is restated in the test.
#include <algorithm>
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

}  // extern "C"
