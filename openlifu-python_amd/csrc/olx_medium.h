// Pure host preparation of float32 medium volumes ([nx][ny][nz], z fastest) for kernels 1m, 1a, 2h / 2m, 2ph, 4h: no HIP, no context, no environment.
// olx.hip keeps the state checks, the error text and the device buffers; tools/medium_check.cpp compares every output of this unit bit for bit with a
// per-voxel restatement under g++ -fsanitize=address,undefined (tests/test_medium_prep_host.py, no GPU).
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>
#include "../../include/olx.h"
namespace olxmed {
// which rule failed (the caller words the message); axis by axis, sizes >= 1 first, then spacing finite and > 0, origin finite
enum GridFault { GRID_OK = 0, GRID_SIZE, GRID_SPACING };
GridFault check_grid(const olx_grid& g);
// index of the first voxel that breaks the rule (NaN breaks both; +inf only where `finite` is asked for), n when none does or the volume is null
enum Rule { POSITIVE, NON_NEGATIVE };
size_t first_bad(const float* v, size_t n, Rule rule, bool finite = true);
// volumes checked voxel by voxel: which of their first_bad indices wins -- the lowest, ties to the earlier entry; -1 when all equal n
int first_bad_volume(const size_t* bad, int m, size_t n);
// dB/cm/MHz^y -> Np, each in the association order of the kernel that first used it (the doubles differ in the last bit)
constexpr double DB_PER_NP = 8.685889638065035;
inline double np_per_m(double db_cm, double fpow) { return db_cm * fpow * 100.0 / DB_PER_NP; }      // one value, fpow = (f / MHz)^y (kernel 1a)
inline double np_per_m_factor(double freq_hz, double power) { return std::pow(freq_hz * 1e-6, power) * 100.0 / DB_PER_NP; }      // Np/m (2ph; times lambda: 4h)
inline double np_per_wavelength_factor(double freq_hz, double power, double lambda) { return std::pow(freq_hz * 1e-6, power) * 100.0 * (1.0 / DB_PER_NP) * lambda; }      // (2h / 2m)
// THE non-trivial-plane rule: plane k is held when any of its voxels has (double)sound_speed != c_ref or attenuation != 0.f (either may be null)
struct Planes { std::vector<int> plane_of_k, plane_k; };     // [nz] plane index or -1 | [np] k, ascending
Planes scan_planes(const float* sound_speed, double c_ref, const float* attenuation, int nx, int ny, int nz);
// kernels 1m / 1a: the planes of ONE volume (the sound speed if given, else the attenuation) and, appended to `col` as soon as a plane is found held, while
// the scan's cache lines are still near, its [i][j] column in fp64: sigma = c_ref / c - 1, or a = np_per_m(value, fpow) [Np/m]
Planes scan_planes_columns(const float* sound_speed, double c_ref, const float* attenuation, double fpow, int nx, int ny, int nz, std::vector<double>& col);
// per element: first plane strictly above its z, last plane strictly below (fp64, z_k = oz + k hz: the predicate the oracle shares)
struct Bounds { std::vector<int> kfirst, klast; };
Bounds element_plane_bounds(const double* ez, int n, double oz, double hz, int nz);
// compact [plane][i][j] columns of kernel 2ph: sigma = c_ref / c - 1 in fp64, a = value x afac rounded once
std::vector<double> plane_sigma(const float* sound_speed, double c_ref, size_t nxy, int nz, const std::vector<int>& plane_k);
std::vector<float> plane_att(const float* attenuation, double afac, size_t nxy, int nz, const std::vector<int>& plane_k);
// the pre-gathered bilinear stencil: texel (p, i, j) = { sigma, a' } of (i, j), (i, j+1), (i+1, j), (i+1, j+1), edge-clamped, max(planes, 1) planes
// long, from cell = [planes][nx][ny] { sigma, a' }: the held planes' own (float)(c_ref / c - 1), (float)(attenuation afac) (0 where the volume is
// null), or their column sums over layers [lo, hi] of planes (fp64 sums, rounded once)
std::vector<float> gather_stencil(const std::vector<float>& cell, int planes, int nx, int ny);
std::vector<float> plane_cells(const float* sound_speed, double c_ref, const float* attenuation, double afac, size_t nxy, int nz, const std::vector<int>& plane_k);
std::vector<float> layer_cells(const float* sound_speed, double c_ref, const float* attenuation, double afac, size_t nxy, int nz, const std::vector<int>& layer_lo, const std::vector<int>& layer_hi);
// two-level quadrature: every maximal run of consecutive held planes is cut into layers of <= G planes
void layer_runs(const std::vector<int>& plane_k, int G, std::vector<int>& layer_lo, std::vector<int>& layer_hi);
// kernel 2m's one-sum form: every texel's own { sigma, a' } on ONE line through the origin (fp64 products of the stored floats); (s_ref, a_ref) =
// the first pair that is not (0, 0); the form holds when `one` and s_ref != 0
struct OneLine { bool one; double s_ref, a_ref; };
OneLine detect_one_line(const std::vector<float>& med, size_t cells);
// per-voxel 1e-4 / (2 rho c) of the intensity over voxels [off, off + count); a null volume stands for its scalar
std::vector<float> impedance_volume(const float* density, double rho0, const float* sound_speed, double c0, size_t off, size_t count);
}  // namespace olxmed
