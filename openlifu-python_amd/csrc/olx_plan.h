// Pure host planning of kernel 2: lattice detection, K-slot map, mirror permutations, column packing, store-target balancing, block records,
// store-job lists, focus inference, the e4m3 rule (fp8_first_plane, fp8_split_pays), kernel 2f's block shape (toep_plan) -- and the DECISION that
// combines them: decide_variant chooses among the eleven field kernels (2a .. 2g, 2h / 2m), their shapes and parameter blocks, and names the variant.
// No HIP, no device memory, no context, no environment: plain C++17 in, plain vectors out.  olx.hip (configure_variant) reads the pins, calls
// decide_variant and uploads what it returns; the SAME translation unit is compiled with g++ -fsanitize=address,undefined into the CPU-side
// checker tools/plan_check.cpp, which `pytest -m "not gpu"` drives over fuzz shapes (tests/test_plan_host.py: every (focus, image) stored exactly
// once, every voxel covered exactly once, records inside the grid, the kernels' magic divisions exact, the e4m3 rule's known decisions and refusals,
// kernel 2f's known shapes, the decision's flags, tables and record key consistent with each other), and into tools/plan_query.cpp, through which
// the parity matrices compare the variant string of every row with the one they expect -- the planning AND the decision run without a GPU.
#pragma once
#include <string>
#include <vector>

#include "olx_params.h"

namespace olxplan {

using olx::CosetBlock;
using olx::CosetParams;

// a matrix array on a regular (a, b) lattice in one z plane whose pitch is a whole number of voxels (kernel 2d's precondition)
struct Lattice {
    bool ok = false;
    int ax = 0, ay = 0, nsa = 0, nsb = 0, mx = 1, my = 1, n_pad = 0;
    double x0 = 0, y0 = 0, px = 0, py = 0;     // position of lattice index (0, 0) and pitch [m]
    double min_d2 = 0; bool clamp = false;     // incl. the zero-weight virtual elements of the padding
    std::vector<int> slot_elem;                // K slot -> element (-1 = virtual)
    std::vector<int> cell;                     // lattice cell (a, b) -> element
    int nsbp = 0;                              // super-block rows of the slot map (nsb, or nsb padded to even)
};

// K-slot map: slot ((sa nsbp + sbb) 4 + ks) 16 + 4 bb + aa -> element (a, b) = (8 sa + 4 (ks & 1) + aa, 8 sbb + 4 (ks >> 1) + bb), -1 where
// the array has no element.  sa-major; nsbp = nsb, or nsb padded to an even count for the shapes that share one table per pair.
void build_slot_map(Lattice& L, int nsbp);

// pos = [3][n] element positions [m] (SoA), lo / hi = bounding box of the planned slab [m], dmin = clamp distance [m]
void detect_lattice(Lattice& L, bool flat, int n, const double* pos, const double spacing[3], const double lo[3], const double hi[3], double dmin);

// MFMA row tiles (16 rows) one plane pair of kernel 2e needs over all cosets and parts
long long coset_tiles16(int wx, int wy, int mx, int my, int nt);

// Element permutations of the mirror images, [rows][n]: image m < n_img folds x (bit 0, where fold_x) and / or y (the next bit) through the
// axis permutations px / py (read only where their axis is folded); rows from n_img on are the identity.
std::vector<int> mirror_perms(int n, int n_img, bool fold_x, bool fold_y, const int* px, const int* py, int rows);

// A column = one distinct steering vector W[sigma_m(e), f]; every (focus, mirror image) whose vector equals it is a store TARGET of
// that column (code = focus * 4 + image), at most 4 per column.
struct Col { int f, m, ntgt; int tgt[4]; };
typedef std::vector<std::vector<Col>> Tiles;

struct Steering {           // what the column plan reads
    int n = 0, F = 0, n_img = 1;
    const int* perm = nullptr;        // [4][n] element permutation of mirror image m
    const double* delays = nullptr;   // [F][n] s
    const double* apod = nullptr;     // [F][n]
    const double* area = nullptr;     // [n]
    double freq = 0;
};
bool same_vector(const Steering& S, int f1, int m1, int f2, int m2);
// greedy packing into launch tiles of at most maxc columns; an equal vector is looked for in EVERY tile packed so far
Tiles pack_columns(const Steering& S, int maxc);
// kernel 2g stores per column slot: a column with 3 - 4 targets hands half of them to a free slot of its tile (same weights)
void balance_store_targets(Tiles& tiles, int max_cols);

// parts the cosets' position grids are cut into (at most kxw x kyw positions per part) and plane blocks of zb planes: Q.nsx, Q.nsy, Q.kblocks
// from Q.nx, ny, nz, x_lo, y_lo, mx, my
void coset_partition(CosetParams& Q, int kxw, int zb, int kyw = olx::COS_KYW);

// Block records of kernels 2e / 2f / 2g: blockIdx.x -> (coset, part, plane block).  zb = planes per block, grp = blocks that share
// 128-byte output lines (ids 8 apart = one XCD).  Returns false (msg) when a part exceeds max_pos positions (0 = no limit).
// heavy_first (kernel 2g): the position sets in the order of falling position count (stable) instead of the coset order.
bool build_coset_blocks(const CosetParams& Q, int zb, unsigned grp, int max_pos, std::vector<CosetBlock>& blk, std::string& msg, bool heavy_first = false);

// dense store-job lists of kernel 2e per (launch tile, column tile): job = c16 | image << 4 | focus << 6; entry [jobs_per_tile] = log2 ceil
std::vector<int> build_store_jobs(const Tiles& tiles, int max_nt, int cols_per_nt, int jobs_per_tile, bool want_p, bool want_i);

// foci of geometric delays (tau_e = max tof - tof_e) on a flat array by linear trilateration; accepted only if every delay is reproduced to 1 um
bool infer_foci(bool flat, int n, int F, const double* pos /*[3][n]*/, const double* delays /*[F][n]*/, double c, double grid_z_mid,
                std::vector<double>& foci);

// ---- error bound of the e4m3 correction products (kernels 2e / 2f / 2g; calibration: tools/emul_fp8_bound.py) ----
// The scheme's error is RELATIVE TO EACH TERM w_e G(v, e): sigma_1 = 6.2e-6 |w_e| / d'(v, e) per element with random sign (<= 2^-13 worst case),
// so a voxel v carries  err(v) <= FP8_ERR_K sqrt(S2(v)),  S2(v) = sum_e (w_e / d'(v, e))^2, with FP8_ERR_K = 6 sigma_1 (the largest
// normalised error over 3.4 M emulated voxels x 8 foci of every scenario was 5.7 - 6.4 sigma_1).  Far from the array that is the
// 1 / sqrt(N_eff) of the focal peak of round 5's argument; NEXT to an element the single nearest term dominates S2 and the error
// can exceed the focal peak's share (grids through / close above the element plane: VERDICT round 5).  The planner therefore asks for
//     FP8_ERR_K * wmax_f * sqrt(max_v sum_e 1 / d'(v, e)^2) <= FP8_ERR_BOUND * sum_e w_ef / d(focus_f, e)      for every focus f
// (right side: the coherent focal peak, a lower bound of the volume maximum when the focus lies inside the planned volume) and keeps
// three fp16 products otherwise -- for the whole launch, or (round 6) for the plane blocks below the first one from which the rule holds.
// Voxels ON a symmetry plane of the array see element pairs at identical distances, whose errors add coherently: the caller raises
// FP8_ERR_K by a quarter per symmetry plane that carries voxels (fp8_first_plane below; calibration in tools/emul_fp8_bound.py).
constexpr double FP8_ERR_K = 3.75e-5;        // 6 sigma_1
constexpr double FP8_ERR_BOUND = 7.5e-6;     // stated in include/olx.h (olx_field_plan); north_star's gate is 1e-5
// max over the candidate voxels (the voxel of the planned slab nearest to each element: S2 peaks next to an element) of
// sum_e 1 / max(d(v, e), dclamp)^2 [1/m^2].  pos = [3][n] (SoA) [m]; voxel i of axis a sits at origin[a] + i spacing[a], i in [begin[a], begin[a] + count[a]).
// O(n * min(n, 1024)): evaluated once per (element table, planned slab) by the caller.
double nearfield_s2(int n, const double* pos, const double origin[3], const double spacing[3], const int begin[3], const int count[3], double dclamp);

// The rule itself.  Returns the first plane of the e4m3 products (0: every plane; a multiple of COS_ZB = the plane blocks of kernels 2e / 2f / 2g: the
// blocks below keep three fp16 products), or -1: not eligible.  (i) every focus lies inside the planned SLAB [x_begin, x_begin + x_count) x ny x nz,
// (ii) has N_eff = (sum w)^2 / sum w^2 >= 256, and (iii) the near-field condition above holds for the planes from the cut on -- the error of a voxel
// belongs to the arithmetic its OWN plane block runs, and it is measured against the maximum of the whole volume, which holds the focal peak by (i).
// pos = [3][n] (SoA) [m], area = [n], apod = [F][n], foci = [F][3] [m] (known: the caller resolves them); L: the array's lattice (x0, px, ax, y0, py, ay:
// where its symmetry planes lie).  nf_s2 = [plane block q] nearfield_s2 of the planes >= COS_ZB q (< 0 = not derived yet): the caller's cache, filled
// lazily here, valid for one (element table, planned slab).
int fp8_first_plane(int n, const double* pos, const double* area, const double* apod, int F, const double* foci, const double origin[3],
                    const double spacing[3], const int gn[3], int x_begin, int x_count, const Lattice& L, std::vector<double>& nf_s2);
// whether a launch split at plane `cut` > 0 (fp16 x 3 below, e4m3 from it on) beats three fp16 products throughout
bool fp8_split_pays(int x_count, int ny, int nz, int F, int cut);

// ---- kernel 2f's block shape (k_toep.hip.h, ToepShape<NM>) ----
struct ToepPlan {
    int saw, nsa;            // element super-block width along x, super-block columns (nsa > 16: ks_mask cannot hold them -- the masks stay 0, the caller fails)
    int nm, kyw;             // row tiles of 8 x positions per block, y positions per block
    unsigned ks_mask;        // bit (2 sa + s): K-step s of column sa carries non-zero weights
    int ksteps_total;        // non-zero K-steps over the columns
    int e4_units;            // matrix units of the e4m3 instructions per element row and y position, over the columns
};
// ax = elements along x, mx / my = pitch [voxels], xs = pitches between two positions of a coset along x, wx x wy x nz = computed region [voxels];
// dir_lattice: the DIR instantiations (no three-tile shape); saw_pin (8 .. 24) / nm_pin (1 | 3) override the choice for A/B runs, 0 = none
ToepPlan toep_plan(int ax, int mx, int my, int xs, int wx, int wy, int nz, bool dir_lattice, int saw_pin = 0, int nm_pin = 0);

// ---- the kernel-2 variant decision ----
// Bits of the plan flags the decision reads (include/olx.h: OLX_OUT_PMAG, OLX_OUT_INTENSITY, OLX_OUT_COMPLEX, OLX_FIELD_FP16_CORRECTION; olx.hip asserts the values)
constexpr unsigned FLAG_OUT_PMAG = 1u, FLAG_OUT_INTENSITY = 2u, FLAG_OUT_COMPLEX = 4u, FLAG_FP16_CORRECTION = 32u;

// What the caller read from the environment.  A product build fills `family` and fp8 = -1 only; the rest are the A/B pins of developer builds (OLX_DEV_PINS).
enum class FamilyPin { none, lattice, lattice2d, other };      // OLX_FIELD_VARIANT: unset, "lattice", "lattice2d", any other value
struct Pins {
    FamilyPin family = FamilyPin::none;
    int fp8 = 0;                               // OLX_FP8_CORRECTION: -1 = "0" (opts out like the plan flag), 0 = unset, 1 = forced past the e4m3 rule
    int toep_saw = 0, toep_nm = 0;             // OLX_EXP_TOEP_SAW (8 .. 24), OLX_EXP_TOEP_NM (1 | 3); 0 = none
    int kgrp = 0;                              // OLX_EXP_KGRP (>= 1); 0 = none
    bool cp_noreuse = false, cp_nofillahead = false;      // OLX_EXP_CP_NOREUSE, OLX_EXP_CP_NOFILLAHEAD
    bool cp_nosort = false;                    // OLX_EXP_CP_NOSORT: kernel 2g's position sets in the coset order, not heaviest first
};

// What olx_field_plan established and what the steering provides: values and read-only arrays
struct VariantIn {
    int n = 0, F = 0;
    const double* pos = nullptr;               // [3][n] (SoA) [m]
    const double* area = nullptr;              // [n]
    const double* delays = nullptr;            // [F][n] s (null: no host copy of the steering table)
    const double* apod = nullptr;              // [F][n]
    const int* px = nullptr; const int* py = nullptr;      // [n] axis mirrors of the element set (read where mx / my == 2)
    double freq = 0, c = 0, p0_pa = 0;
    double origin[3] = {0, 0, 0}, spacing[3] = {0, 0, 0}; int gn[3] = {0, 0, 0};      // the grid
    int x_begin = 0, x_count = 0;              // the slab
    unsigned flags = 0;                        // plan flags (FLAG_*)
    olx::FieldParams fp{};
    bool flat = false, clamp = false, near = false;
    double min_dist = 0;                       // lower bound of any voxel-element distance [m]
    int mx = 1, my = 1;                        // mirror folds of the geometry
    bool allow_shared = true, dir_lattice = false, directivity = false;
    double absorb_np_m = 0;
    int force_kind = 0;                        // 0 auto, 1 general, 2 shared, 3 mfma, 4 lattice
    double size0 = 0, size1 = 0;               // width / length of element 0 [m] (directivity on a dir_lattice array: all elements are equal)
    bool hetero = false, marched = false, march_one = false;      // heterogeneous medium: what the name needs
    int n_planes = 0, n_layers = 0, planes_per_layer = 1;
    const Lattice* lat = nullptr;
    const double* foci = nullptr;              // [F][3] m where the foci are known, else null
    Pins pins;
    bool modifier() const { return directivity || absorb_np_m > 0; }
};

struct VariantPlan {
    bool use_mfma = false, use_lattice = false, use_coset = false, use_toep = false, use_cosetp = false, fp8corr = false;
    int fp8_kcut = 0;                          // first plane of the e4m3 products (meaningful while fp8corr)
    int mx = 1, my = 1, dx = 1, dy = 1, nf = 1, nt = 1, lat_mt = 4;
    bool allow_shared = true, dir_lattice = false;      // as they end up after the fallback to kernels 2a-d
    std::vector<int> perm;                     // mirror permutations: [4][n] (kernels 2c - 2g), [dx dy][n] (kernel 2b), empty (2a, 2h / 2m)
    Tiles tiles; int total_cols = 0;
    std::vector<int> colinfo;                  // [column][f, m] then [column][4 store targets], tiles x MFMA_COLS x MFMA_MAX_NT columns
    std::vector<int> jobs;                     // build_store_jobs (use_coset)
    ToepPlan toep{0, 0, 1, olx::COS_KYW, 0u, 0, 0};
    int n_pad = 0; bool lat_clamp = false;
    double g_scale = 0, out_scale = 0, mfma_wscale = 0;
    olx::MfmaParams mp{}; olx::LatParams lp{}; olx::CosetParams cp{};
    unsigned kgrp = 1, kgrp_near = 0;          // plane blocks of one position set in a row per XCD, above / below the cut
    unsigned blocks_near = 0;                  // block records of the plane blocks below the cut (they follow the others)
    bool heavy_first = false;                  // kernel 2g: the position sets of the block records in the order of falling position count
    int rec_key[17] = {0};                     // everything build_variant_blocks reads: the caller rebuilds its block records only when this changes
    long long n_mfma = 0, n_dense = 0;
    std::string variant;
};

// dx / dy: whether every focus' delays and apodization are symmetric under the element permutation of a folded axis
bool steering_symmetric(int n, int F, const double* delays, const double* apod, const double* area, double freq, const int* perm);
// whether decide_variant will ask the e4m3 rule, i.e. read in.foci (the caller resolves them only then: infer_foci)
bool variant_reads_foci(const VariantIn& in);
// The decision.  nf_s2 and slot_rows are the caller's caches: fp8_first_plane's near-field sums, and the rows of the K-slot map the lattice holds
// (in: in.lat->nsbp; out: what the chosen shape needs -- the caller rebuilds the map when it differs; LatParams / CosetParams carry the new count).
VariantPlan decide_variant(const VariantIn& in, std::vector<double>& nf_s2, int& slot_rows);
// The block records of a use_coset plan: those of the plane blocks from the cut on first, then the blocks below it.  False (msg) as build_coset_blocks.
bool build_variant_blocks(const VariantPlan& p, std::vector<CosetBlock>& blk, std::string& msg);

}  // namespace olxplan
