/*
 * olx.h -- C ABI of the MI355X-native openlifu beamforming + pressure-field path.
 *
 * Plain C types only, caller-allocated outputs, no callbacks, no torch types.
 * Every entry point returns 0 on success and a negative OLX_E* code on failure;
 * olx_last_error(ctx) then holds a human-readable message.  One caller thread
 * per context (the reference is synchronous and single-threaded,
 * src/openlifu/plan/protocol.py:318-339); different contexts are independent.
 *
 * The reference is pure Python, so "what its FFI for this path would bind" is
 * the set of Python seams of SURVEY.md 8(b).  Each entry point cites the
 * reference interface it stands in for (paths under /root/reference/src/openlifu).
 * The ctypes binding a maintainer would add is shown in INTEGRATION.md and lives
 * in openlifu-python_amd/openlifu_amd/_native.py.
 *
 * Units are SI throughout: metres, seconds, Hz, Pa, kg/m^3, m/s.  Arrays are
 * C-order.  Field volumes are [nx, ny, nz] with z fastest -- the layout of the
 * arrays run_simulation returns (sim/kwave_if.py:131-139).
 */
#ifndef OLX_H
#define OLX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OLX_ABI_VERSION 2

/* error codes */
#define OLX_OK 0
#define OLX_EINVAL (-1)  /* bad argument (NULL, non-positive size, shape mismatch) */
#define OLX_ESTATE (-2)  /* call order: elements / steering / plan missing */
#define OLX_EHIP (-3)    /* HIP runtime error (message has hipGetErrorString) */
#define OLX_ENOMEM (-4)  /* device or host allocation failed */
#define OLX_ECOMM (-5)   /* RCCL error or RCCL unavailable */
#define OLX_ENOCONV (-6) /* an iteration did not converge within its cap (olx_eikonal_solve); nothing partial is kept */

/* apodization kinds: bf/apod_methods/{uniform,maxangle,piecewiselinear}.py */
#define OLX_APOD_UNIFORM 0   /* p0 = value                              (uniform.py:21-22) */
#define OLX_APOD_MAXANGLE 1  /* p0 = max angle [deg], inclusive <=      (maxangle.py:33-39) */
#define OLX_APOD_PIECEWISE 2 /* p0 = zero angle, p1 = rolloff [deg]     (piecewiselinear.py:42-49) */
#define OLX_APOD_RADIANS 0x10 /* OR-ed into the kind: p0 / p1 are radians (the methods' `units` field) */

/* field output selection (olx_field_plan flags) */
#define OLX_OUT_PMAG 1u      /* |p| [Pa]  -> p_max and p_min of kwave_if.py:131-139 */
#define OLX_OUT_INTENSITY 2u /* 1e-4 |p|^2 / (2 rho c) [W/cm^2]  (kwave_if.py:140-144) */
#define OLX_OUT_COMPLEX 4u   /* (re, im) interleaved, float32 */
#define OLX_OUT_PMAX 64u     /* pulsed plans (olx_field_pulse) only: also keep the peak positive pressure p_max [Pa] (olx_field_fetch_pmax) */
#define OLX_OUT_PII 128u     /* pulsed plans only: also keep the pulse intensity integral 1e-4 dt / (rho c) sum_k p(t_k)^2 [J/cm^2] (olx_field_fetch_pii) */
/* accuracy / speed options of olx_field_plan (OR-ed into flags; see the accuracy note there) */
#define OLX_FIELD_FP8_CORRECTION 8u   /* accepted for source compatibility: asks for what is the default since ABI v2 */
#define OLX_FIELD_FP16_CORRECTION 32u /* opt out of the e4m3 correction products: three fp16 products everywhere (<= 2e-6) */
/* physics option of olx_field_plan (OR-ed into flags): optional far-field piston directivity, SURVEY.md 8(c) "flagged v1"; needs
 * olx_set_element_apertures.  Served by the exact per-pair kernel only (kernel 2a-d). */
#define OLX_FIELD_DIRECTIVITY 16u

typedef struct olx_ctx olx_ctx;

/* Regular grid = the three coordinate vectors of SimSetup.get_coords
 * (sim/sim_setup.py:107-116): coord[a][i] = origin[a] + i * spacing[a]. */
typedef struct olx_grid {
    double origin[3];  /* metres, position of voxel (0,0,0) */
    double spacing[3]; /* metres, > 0 */
    int32_t n[3];      /* nx, ny, nz >= 1 */
} olx_grid;

/* Slab of a grid (multi-GPU sharding along x, the slowest axis): voxels
 * [x_begin, x_begin + x_count) x ny x nz form one contiguous block. */
typedef struct olx_slab {
    int32_t x_begin;
    int32_t x_count;
} olx_slab;

/* ---- library / context --------------------------------------------------------- */
int olx_abi_version(void);
/* Number of visible HIP devices (stands in for util/checkgpu.py:6-14 gpu_available,
 * which is NVML-only and always False on AMD). */
int olx_device_count(int *count);
int olx_ctx_create(int device, olx_ctx **out);
int olx_ctx_destroy(olx_ctx *ctx);
const char *olx_last_error(const olx_ctx *ctx);
int olx_sync(olx_ctx *ctx);

/* ---- element table ------------------------------------------------------------------
 * SoA flattening of Transducer.elements (xdc/element.py:33-59, xdc/transducer.py:203-207):
 * pos_m[N*3] = Element.get_position(units="m"), normal[N*3] = column 2 of
 * Element.get_matrix (element.py:200-214), area_m2[N] = Element.get_area("m")
 * (element.py:181-184).  Order = Transducer.elements order (bit-exact indexing). */
int olx_set_elements(olx_ctx *ctx, const double *pos_m, const double *normal,
                     const double *area_m2, int n);
/* Element apertures for OLX_FIELD_DIRECTIVITY (the reference's sources are finite rectangles for k-Wave, kwave_if.py:34-46
 * add_rect_element; this path's point-source sum can carry their far-field pattern instead):
 *   D_e(v) = sinc(pi w u_x / lambda) sinc(pi l u_y / lambda),  sinc(t) = sin(t)/t,
 * u_x, u_y = direction cosines of r_v - r_e along the element's local x axis (xaxis[N*3] = column 0 of Element.get_matrix) and
 * y axis (normal x xaxis), formed with the clamped distance; size_m[N*2] = (w along x, l along y) = Element.get_size("m").
 * Call after olx_set_elements (which clears them).  Definition: oracle/field_oracle.py piston_directivity. */
int olx_set_element_apertures(olx_ctx *ctx, const double *xaxis, const double *size_m);

/* ---- kernel 1: delay / apodization solve --------------------------------------------
 * DelayMethod.calc_delays (bf/delay_methods/direct.py:28-38) and
 * ApodizationMethod.calc_apodization for F foci in one launch; replaces the F x N
 * Python loops of Protocol.beamform (plan/protocol.py:129-132, 318-320).
 *   foci_m[F*3]  focus positions, metres (Point.get_position(units="m"))
 *   M[16]        row-major 4x4 `transform` (NULL = identity); applied to the element
 *                position for the distance (element.py:241-244) and to position and
 *                normal for the angle (element.py:250-253)
 *   c            speed of sound: params['sound_speed'].attrs['ref_value'] if params
 *                else Direct.c0 (direct.py:29-32)
 * Outputs (host, fp64, caller-allocated [F*N]): delays [s] = max(tof) - tof, apod.
 * Either output pointer may be NULL.  The results also stay device-resident as the
 * context's steering table (consumed by olx_field_*). */
int olx_bf_solve(olx_ctx *ctx, const double *foci_m, int n_foci, const double *M, double c,
                 int apod_kind, double p0, double p1, double *delays_out, double *apod_out);

/* Times `iters` repeats of the last olx_bf_solve's kernel (same foci / transform / options, results rewritten with
 * equal values) with HIP events on the context's stream; us_each[iters] = microseconds per F x N solve (bench.py). */
int olx_bf_time(olx_ctx *ctx, int iters, float *us_each);

/* ---- kernel 1m: StraightRay delays through a medium (DESIGN.md section 2 "StraightRay") --------------
 * The DelayMethod.calc_delays seam again (its `params` argument carries the medium): the delays that make
 * the straight-ray field model of olx_field_set_medium (section 7) add up in phase at each focus,
 *   tau_e = tof_e + E_e / c_ref,   delays = max_e tau_e - tau_e,
 * tof_e = kernel 1's |focus - g_e| / c_ref, E_e = the straight-ray extra path through sigma = c_ref / c - 1.
 * Set the medium: sound_speed [nx*ny*nz] floats on `grid` (C order; NULL = c_ref everywhere), in the frame
 * of the foci.  Only the planes with some sound speed != c_ref are held, in buffers of their own: a field
 * plan, its medium and its volumes are left as they are.  Refused (nothing on the device touched): c_ref
 * non-finite or <= 0, a sound speed non-finite or <= 0, a bad grid. */
int olx_bf_set_medium(olx_ctx *ctx, const float *sound_speed, const olx_grid *grid, double c_ref);
/* olx_bf_solve's arguments and outputs with the delays corrected through the medium of olx_bf_set_medium
 * (c must equal its c_ref); the apodization is kernel 1's.  All foci in one launch; the results stay
 * device-resident as the context's steering table, like olx_bf_solve's.  OLX_ESTATE before a medium is set. */
int olx_bf_solve_medium(olx_ctx *ctx, const double *foci_m, int n_foci, const double *M, double c,
                        int apod_kind, double p0, double p1, double *delays_out, double *apod_out);

/* ---- kernel 1a: MediumCompensated apodization through a medium (DESIGN.md section 2 "MediumCompensated") ----
 * The ApodizationMethod.calc_apodization seam with its `params` argument read: amplitudes that know the attenuation
 * every element's straight ray crosses on its way to the focus,
 *   h_e = exp(-A_e) [S_e / max(d_e, dmin) with spreading],  A_e = the straight-ray sum of section 7 over a [Np/m],
 *   apod_e = b_e (min_active h / h_e)  (OLX_COMP_EQUALIZE)   or   b_e (h_e / max_active h)  (OLX_COMP_MATCHED),
 * b = kernel 1's apodization, active = { b_e > 0 }, S_e = area_m2 of olx_set_elements.  Set the attenuation:
 * attenuation_db_cm_mhz [nx*ny*nz] floats on `grid` (C order; NULL = none), in the frame of the foci, converted at
 * freq_hz with the field model's power law (a = alpha f_MHz^0.9 100 / 8.685889638065035 Np/m, fp64).  Only the planes
 * with some attenuation != 0 are held, in buffers of their own: a field plan, its medium and its volumes, and the
 * medium of olx_bf_set_medium are left as they are.  Refused (nothing on the device touched): freq_hz non-finite
 * or <= 0, an attenuation negative or non-finite, a bad grid. */
enum { OLX_COMP_EQUALIZE = 0, OLX_COMP_MATCHED = 1 };
int olx_bf_set_attenuation(olx_ctx *ctx, const float *attenuation_db_cm_mhz, const olx_grid *grid, double freq_hz);
/* olx_bf_solve's arguments and outputs with the apodization compensated through the attenuation of
 * olx_bf_set_attenuation; use_delay_medium != 0: and the delays corrected through the medium of olx_bf_set_medium
 * (olx_bf_solve_medium's, bit for bit; c must equal its c_ref and both media must share one grid), both by ONE walk
 * of the rays.  Without attenuation on any ray and without spreading the apodization is kernel 1's bit for bit.  An
 * h_e that underflows to 0 (A_e > 700) is outside the method's range.  The results stay device-resident as the
 * steering table.  OLX_ESTATE before an attenuation (and, with use_delay_medium, a medium) is set; olx_bf_time is
 * refused after it, as after olx_bf_solve_medium. */
int olx_bf_solve_compensated(olx_ctx *ctx, const double *foci_m, int n_foci, const double *M, double c,
                             int apod_kind, double p0, double p1, int mode, int spreading, int use_delay_medium,
                             double *delays_out, double *apod_out);

/* Upload externally computed delays / apodizations [F*N] as the steering table
 * (run_simulation's `delays`, `apod` arguments, sim/kwave_if.py:81-83, 98-99). */
int olx_set_steering(olx_ctx *ctx, const double *delays_s, const double *apod, int n_foci);

/* Hardware hand-off of the resident steering table: what LIFUTXDevice.set_solution derives per
 * focus before it packs registers (io/LIFUTXDevice.py:1357-1372): ticks[F*N] = int(delay * 1.0 * bf_clk) (the
 * reference's fp64 expression, :1874, truncated toward zero -- bit-exact), apod_off[F*N] = int(1 - apod) (the
 * apodization register bit, :1811), max_apod[F] (duty_cycle = 0.66 * max(apod) * amplitude, :1358) and
 * n_overflow[F] = delays that do not fit width_bits (DELAY_WIDTH = 13; set_register_value raises, :1500).
 * Any output pointer may be NULL.  Register addresses / bit positions are device tables and stay in openlifu. */
int olx_bf_quantize(olx_ctx *ctx, double bf_clk_hz, int width_bits, uint16_t *ticks_out,
                    uint8_t *apod_off_out, double *max_apod_out, int32_t *n_overflow_out);

/* ---- kernel 2: pressure-field accumulate --------------------------------------------
 * Stands in for run_simulation (sim/kwave_if.py:80-146) at the seam
 * plan/protocol.py:324-336.  Steady-state monochromatic point-source superposition
 * (definition: oracle/field_oracle.py):
 *   p_f(v) = sum_e a_ef P0 S_e / (lambda d) exp(j (k d + 2 pi f0 tau_ef)),
 *   d = max(||r_v - r_e||, min(spacing)/2).
 * plan: fixes grid / medium / outputs and allocates device buffers for n_foci volumes
 *   (n_foci must equal the steering table's F).  p0_pa = amplitude * sensitivity
 *   (xdc/transducer.py:105-106), rho/c = reference medium values (kwave_if.py:52-56).
 * launch: asynchronous on the context's stream.  fetch: blocking D2H of one focus
 *   volume into caller-owned host arrays [nx*ny*nz] (cplx: 2 floats per voxel); any
 *   pointer may be NULL.
 * accuracy: fp32 results within 1e-5 of the volume's maximum |p| against the fp64 definition (north_star's gate; the
 *   per-pair and fp16-split kernels measure 0.8e-6 ... 2.1e-6, also on grids through the element plane: wherever a voxel comes
 *   within a quarter wavelength of an element they form voxel - element differences from exact index differences, not from
 *   rounded absolute coordinates).  Matrix arrays on a commensurate grid (the lattice
 *   kernels 2e / 2g and the single-column kernel 2f) compute the two small correction products of their fp16 hi/lo
 *   operand split in fp8 (e4m3) BY DEFAULT -- ~20 % faster, error <= 7.5e-6 of the VOLUME MAXIMUM (measured 4.1e-6 ...
 *   6.2e-6 on full 256^3 volumes) -- but only where the planner can bound it (olx_plan.h, FP8_ERR_K / FP8_ERR_BOUND):
 *   the scheme's error is relative to each element's own term, 6.2e-6 |w_e| / d(v, e) rms with random sign, so it asks for
 *     (i)   every focus of the steering table known (it came from olx_bf_solve in the element frame, or its external
 *           delays are recognised as geometric) and inside the planned slab -- the slab then holds the coherent focal
 *           peak P_f = sum_e w_ef / d(focus_f, e);
 *     (ii)  >= 256 effectively driven elements, (sum w)^2 / sum w^2;
 *     (iii) 3.75e-5 s max_e(w_ef) sqrt(max_v sum_e 1 / d'(v, e)^2) <= 7.5e-6 P_f for every focus: six sigma of the error of the
 *           WORST voxel (the one next to an element; d' = the clamped distance), the maximum taken over the planes that run
 *           the e4m3 products; s = 1, 1.25 or 1.5 with voxels on none, one or both symmetry planes of the array (element
 *           pairs at identical distances: their errors add coherently).  The kernels work in blocks of 16 planes, and the
 *           rule is asked per block: a launch is SPLIT at the first plane block from which it holds -- three fp16 products
 *           below ("fp8corr from plane K" in olx_field_variant; those planes carry the opted-out plan's bits), e4m3 above.
 *           A split is two launches: it is taken only while >= 3/4 of the planes lie above the cut and >= 8 M (voxel, focus)
 *           pairs do; otherwise the whole launch keeps three fp16 products.  On BASELINE's 16 x 16 array: every plane for grids
 *           that start >= ~4.5 mm above the element plane; a 240 x 240 x 256 grid from z = -4 mm at 0.25 mm is split at plane
 *           32 / 48 (z = 4 / 8 mm); the reference's default SimSetup (odd voxel counts centred on the array: voxels on both
 *           symmetry planes, cut at z = 28 / 20 / 16 mm for 1 / 0.5 / 0.25 mm) runs three fp16 products throughout.
 *   Everything else -- small or strongly apodized arrays, arbitrary delay patterns, slabs beside the foci, the plane
 *   blocks next to the array, 17-32 columns in one tile, complex output -- keeps three fp16 products (<= 2e-6).  OLX_FIELD_FP16_CORRECTION
 *   in `flags` (or OLX_FP8_CORRECTION=0 in the environment) opts out everywhere; nothing can opt IN past the rule in the
 *   product library (OLX_FP8_CORRECTION=1 is honoured by developer builds only).
 *   olx_field_variant() names the kernel in use ("fp8corr" when the e4m3 products are active).
 * intensity (OLX_OUT_INTENSITY): a continuous-wave plan in a homogeneous medium DERIVES it.  Kernel 2 stores |p| only (an intensity-only
 *   plan stores |p| as well), no intensity volumes are reserved, and every reader -- the fetches, the scans, olx_solution_analyze, the
 *   aggregates, olx_field_scale (which then scales |p| only) -- forms I = (|p| * |p|) * k from the float32 |p| as it is stored, k =
 *   (float)(1e-4 / (2 rho c)): two separately rounded fp32 products, the same bits on every path.  The few readers of whole intensity
 *   volumes (olx_field_masked_peak(which = 1), olx_field_sample(which = 1), the resident source of olx_thermal_run) fill such volumes from
 *   |p| on their first call; they stay valid until the next launch, scaling or plan.  Pulsed plans, a heterogeneous medium
 *   (olx_field_set_medium switches the plan back), uploaded results, and any plan made with OLX_INTENSITY_STORED=1 in the environment (read
 *   by olx_field_plan; the pin for same-binary A/B runs and for callers that need the former bits) keep separately stored volumes, written
 *   by kernel 2 as m * s_i from the squared magnitude m.  The two forms differ by rounding only: see olx_field_fetch. */
int olx_field_plan(olx_ctx *ctx, const olx_grid *grid, const olx_slab *slab /*NULL = whole grid*/,
                   int n_foci, double freq, double c, double rho, double p0_pa, unsigned flags);
int olx_field_launch(olx_ctx *ctx);
/* One focus' volumes into caller-owned memory (any may be NULL).  intensity of a launched continuous-wave plan in a homogeneous medium
 * is DEFINED as (|p| * |p|) * k of the float32 |p| this call returns (see olx_field_plan; formed on the device in one volume of scratch, then
 * copied out) -- no longer a separately rounded product of the squared magnitude.  Measured worst relative difference per voxel between the
 * two: 3.9e-7 (kernels 2a / 2e / 2f / 2g, tests/test_gpu_derived_intensity.py; worst-case arithmetic: 6.6e-7), fifty times below the
 * 2e-5 gate against the fp64 definition; |p| is bit-identical. */
int olx_field_fetch(olx_ctx *ctx, int focus, float *pmag, float *intensity, float *cplx);
/* All planned focus volumes at once ([F * slab voxels] floats each, either may be NULL): one pipelined transfer through a
 * ring of pinned chunks whose copy-out into the caller's (pageable, caller-owned) arrays runs on several host threads. */
int olx_field_fetch_all(olx_ctx *ctx, float *pmag, float *intensity);
/* One-shot convenience: plan + launch + fetch of all foci ([F * slab voxels] each). */
int olx_field(olx_ctx *ctx, const olx_grid *grid, int n_foci, double freq, double c, double rho,
              double p0_pa, float *pmag_out, float *intensity_out);

/* Heterogeneous medium for the planned grid (BASELINE config 5; the reference only forwards these
 * volumes to k-Wave, sim/kwave_if.py:58-62): per-voxel sound speed [m/s], attenuation [dB/cm/MHz^y] and
 * density [kg/m^3] of the WHOLE grid, C-order [nx,ny,nz]; any pointer may be NULL (= reference value given
 * to olx_field_plan).  Switches the accumulate to the straight-ray layered model:
 * phase 2 pi f0 (d/c0 + integral (1/c - 1/c0) ds), amplitude x exp(-integral alpha f^y ds), intensity with
 * the voxel's own rho c.  Valid until the next olx_field_plan. */
int olx_field_set_medium(olx_ctx *ctx, const float *sound_speed, const float *attenuation,
                         const float *density, double alpha_power);
/* Quadrature of the ray integrals for the NEXT olx_field_set_medium calls of this context (default 1): with
 * planes_per_layer = G > 1 every run of consecutive non-trivial grid planes is cut into layers of <= G planes and a layer
 * lying wholly between element and voxel is sampled ONCE at its mid height with the column sums of its planes (a thin
 * phase / absorption screen; the planes of the layer a voxel sits in are still sampled one by one).  ~G x fewer gathers
 * per ray; the lateral walk of a ray inside a layer is neglected (per-cent-level change of the field on the skull-slab
 * phantom at G = 8).  Definition: oracle/field_oracle.c olo_field_grid_hetero_layers. */
int olx_field_medium_layering(olx_ctx *ctx, int planes_per_layer);
/* Ray-integral model for the NEXT olx_field_set_medium calls of this context (default OLX_MEDIUM_AUTO):
 *   OLX_MEDIUM_SAMPLED  one bilinear sample on EVERY non-trivial plane between element and voxel (kernel 2h; with
 *                       olx_field_medium_layering > 1 its two-level form).  Definition: olo_field_grid_hetero(_layers).
 *   OLX_MEDIUM_MARCHED  running ray sums carried from one non-trivial plane to the next on the grid, ONE bilinear look-up per
 *                       (voxel, element) (kernel 2m, ~20 x faster on the skull-slab phantom).  Differs from SAMPLED only by the
 *                       re-interpolation of the running sum at each non-trivial plane.  Needs every element strictly below the
 *                       first non-trivial plane, >= 2 voxels along x and y and planes_per_layer = 1; olx_field_set_medium
 *                       fails with OLX_EINVAL otherwise.  Definition: oracle/field_oracle.c olo_field_columns_hetero_march.
 *   OLX_MEDIUM_AUTO     MARCHED when its preconditions hold, else SAMPLED (olx_field_variant names the kernel in use). */
#define OLX_MEDIUM_AUTO 0
#define OLX_MEDIUM_SAMPLED 1
#define OLX_MEDIUM_MARCHED 2
int olx_field_medium_model(olx_ctx *ctx, int model);
/* Uniform absorbing medium for the plans that follow (0 = lossless, the default): sound speed and density are the plan's
 * constants and every term carries exp(-a d), a = np_per_m (the caller converts the reference's dB/cm/MHz^y: alpha f_MHz^0.9 *
 * 100 / 8.686, alpha_power 0.9 as sim/kwave_if.py:57).  A medium that is the same everywhere is homogeneous: this runs on the
 * homogeneous kernels (the lattice kernels' "modified table" instantiations, else the per-pair kernel 2a-d), not on the
 * layered-ray kernels of olx_field_set_medium -- which the absorption a PLAN was made under excludes.  A plan keeps the value it was made under: a later call changes no
 * launch of a plan that stands, whatever steering table that launch runs with.  Example: the reference's example_protocol.json (water
 * with 0.0022 dB/cm/MHz). */
int olx_field_absorption(olx_ctx *ctx, double np_per_m);

/* Pulsed (tone-burst) field model for the plans that follow, the reference's time-domain run (sim/kwave_if.py:100-139 drives every
 * element with `cycles` cycles sampled at `dt` and records the peak pressures up to t_end); n_t = 0 (the default) = the continuous-wave
 * model of every kernel above.  With n_t > 0 the field of focus f is the time-domain Rayleigh sum (kernel 2p)
 *   p(v, t) = sum_e w_e exp(-a d_e) / d_e cos(2 pi f0 (t - t_e)) 1[0 <= t - t_e < cycles / f0],  t_e = floor(tau_e / dt) dt + d_e / c
 * sampled at t_k = k dt, k = 0 .. n_t - 1 (w_e, d_e and a as in the CW model).  The plan's OLX_OUT_PMAG slot then holds the peak negative
 * pressure p_min = max(0, -min_k p) -- what the analysis, the scaling and the intensity 1e-4 p_min^2 / (2 rho c) read -- and
 * OLX_OUT_PMAX asks for p_max = max(0, max_k p) as one more resident volume: olx_field_scale, olx_field_scale_aggregate and the scaling
 * of olx_solution_analyze scale it too, the device aggregate also forms max_f p_max_f (olx_aggregate_fetch_pmax).  Homogeneous media
 * (with olx_field_absorption) and any element geometry; a pulsed plan refuses a slab, a communicator, OLX_FIELD_DIRECTIVITY,
 * OLX_OUT_COMPLEX and olx_field_set_medium (a heterogeneous medium is opt-in: olx_field_pulse_medium below).  cycles > 0 and dt > 0 [s] are used as given (the caller applies its defaults).
 * Two more outputs of the same time axis (neither touches a plan that does not ask for it):
 *   OLX_OUT_PII   the pulse intensity integral PII_f(v) = 1e-4 dt / (rho c) sum_k p_f(v, t_k)^2 [J/cm^2] as one more resident volume
 *                 (olx_field_fetch_pii); PII / (cycles / f0) is the pulse-average intensity [W/cm^2].  olx_field_scale, olx_field_scale_aggregate
 *                 and olx_solution_analyze do NOT scale it and the device aggregate does not aggregate it: olx_pii_post (below) is the
 *                 only thing that scales it (by factor^2 for pressures scaled by `factor`) and forms its sum and maximum over foci.
 *   olx_field_pulse_trace   the waveform p_f(v_i, t_k), k = 0 .. n_t - 1, at chosen voxels. */
int olx_field_pulse(olx_ctx *ctx, double cycles, double dt, int n_t);
/* p_max of every planned focus of the last pulsed launch ([F * voxels] floats), as scaled since. */
int olx_field_fetch_pmax(olx_ctx *ctx, float *pmax_out);
/* max_f p_max_f of the last device aggregate of a pulsed plan's volumes ([voxels] floats). */
int olx_aggregate_fetch_pmax(olx_ctx *ctx, float *pmax_out);
/* Pulse intensity integral of every focus of the last pulsed launch with OLX_OUT_PII, or of olx_pii_upload ([F * voxels] floats, J/cm^2),
 * as scaled since by olx_pii_post (nothing else scales it, see olx_field_pulse). */
int olx_field_fetch_pii(olx_ctx *ctx, float *pii_out);
/* One pass over the resident PII volumes (a pulsed plan with OLX_OUT_PII that has been launched, or olx_pii_upload), at most 8 foci
 * (DESIGN.md section 2 "pulse energy"):
 *   scale_per_focus [F] or NULL   PII_f *= (float)(s_f * s_f) in place (the product in fp64, rounded once; one fp32 multiply per voxel)
 *   weights [F] or NULL           the weighted volume sum_f w_f PII_f (fp32, f ascending, acc = fmaf((float)w_f, PII_f, acc) from 0, over
 *                                 the scaled values): the dose of a pulse train for w_f = pulses aimed at focus f; NULL = no weighted volume
 *   A [F * 12] or NULL            focal frames and masks as olx_field_analysis_peaks (every selection is the fp64 one): peaks_out[F * 4 + 1] =
 *                                 per focus {mainlobe PII, sidelobe PII, global PII, mainlobe weighted}, then the global (z > zmin) peak of
 *                                 the weighted volume (the weighted peaks are 0 without weights); NULL = no peaks, aspect / peaks_out unused
 * and always max_f PII_f.  OLX_ESTATE without resident PII, OLX_EINVAL when n_foci is not the resident volumes' count.  Synchronous. */
int olx_pii_post(olx_ctx *ctx, const double *scale_per_focus, const double *weights, int n_foci,
                 const double *A, const double *aspect, double r_main_m, double r_side_m, double zmin_m, float *peaks_out);
int olx_pii_fetch_weighted(olx_ctx *ctx, float *out);   /* sum_f w_f PII_f of the last olx_pii_post with weights ([voxels] floats); OLX_ESTATE once the PII has been scaled or replaced since */
int olx_pii_fetch_max(olx_ctx *ctx, float *out);        /* max_f PII_f of the last olx_pii_post ([voxels] floats) */
/* Host PII volumes ([n_foci * voxels] floats) onto the grid of the current plan / upload: the resident PII from then on, until the next
 * plan, upload or pulsed launch. */
int olx_pii_upload(olx_ctx *ctx, int n_foci, const float *pii);
/* Waveforms of the current pulsed plan with the current steering table (the plan need not have been launched, and needs no particular
 * output flag): trace_out[(f * n_points + i) * n_t + k] = p_f(voxels[i], t_k) [Pa], float32, for all planned foci; voxels are linear C-order
 * indices of the planned grid (OLX_EINVAL outside it).  A sample at which no element has arrived yet, or after the last burst has ended,
 * is exactly 0.  One wave per (point, focus): meant for tens of points, not for volumes -- more than OLX_PULSE_TRACE_MAX_SAMPLES
 * samples (F * n_points * n_t) in one call give OLX_EINVAL.  Synchronous. */
#define OLX_PULSE_TRACE_MAX_SAMPLES (1ll << 26) /* 256 MiB of float32 */
int olx_field_pulse_trace(olx_ctx *ctx, int n_points, const long long *voxels, float *trace_out);
/* Drive impulse responses for the pulsed plans that follow, like olx_field_pulse (DESIGN.md section 2 "drive taps", kernel 2p's RESP
 * instantiations): the reference's Transducer.calc_output drives element e with the tone burst convolved with the array's and the element's
 * impulse responses resampled to dt.  With the drive taps g_e[m], m = 0 .. M_e - 1, on the dt grid the field is
 *   p(v, t_k) = sum_e w_e exp(-a d_e) / d_e sum_m g_e[m] cos(2 pi f0 (t_k - t_e - m dt)) 1[0 <= t_k - t_e - m dt < T]
 * and p_max, p_min, the intensity, OLX_OUT_PII and olx_field_pulse_trace are formed from it as from the bare burst; n_t is unchanged (ring-down
 * past it is cut).  Elements with identical taps share a class: class_of_element[N] in 0 .. n_classes - 1, the taps of class r are
 * taps[row[r] .. row[r + 1]) (fp64; the kernel takes them as float2 with the carrier's phase e^{-j 2 pi f0 dt m} folded in on the host).
 * A trace is exactly 0 before the first arrival and from the last burst end + M_max - 1 on.  One class with the single tap 1.0 gives
 * the plain plan's volumes bit for bit.  n_classes = 0 clears the response: the plans that follow launch exactly what they launch today.
 * Needs the element table (OLX_ESTATE); olx_set_elements clears it, as it clears the apertures.  OLX_EINVAL, before anything is kept: a
 * class id out of range, a row table that does not start at 0 or is not strictly increasing, more than OLX_PULSE_RESPONSE_MAX_TAPS taps in
 * a class, more than OLX_PULSE_RESPONSE_MAX_CLASSES classes, a tap that is not finite.  Continuous-wave plans ignore it;
 * olx_field_pulse_medium refuses a plan that carries one (kernel 2ph has no response).  olx_field_variant then ends in
 * "; response: R classes, M taps" (M = the longest class). */
#define OLX_PULSE_RESPONSE_MAX_TAPS 256
#define OLX_PULSE_RESPONSE_MAX_CLASSES 4
int olx_field_pulse_response(olx_ctx *ctx, int n_classes, const int32_t *class_of_element, const int32_t *row, const double *taps);
/* Heterogeneous medium for the CURRENT pulsed plan, opt-in (DESIGN.md section 2 "Pulsed model through a medium", kernel 2ph): valid only
 * after olx_field_plan of a pulsed plan (OLX_ESTATE otherwise), until the next olx_field_plan.  Volumes as olx_field_set_medium's: float32
 * [nx*ny*nz] of the whole planned grid, C order, NULL = the plan's constant; attenuation in dB/cm/MHz^alpha_power.  olx_field_launch and
 * olx_field_pulse_trace of the plan then run the pulsed model with the medium on every straight ray (sampled quadrature, one sample per
 * non-trivial plane, plane bounds and ray sums A_e, E_e exactly as olx_steer_map_medium defines them at a grid voxel):
 *   t_e = floor(tau_e / dt) dt + (d'_e + E_e) / c_ref,   p(v, t) = sum_e w_e exp(-A_e) / d'_e cos(2 pi f0 (t - t_e)) 1[0 <= t - t_e < T]
 * p_max, p_min, PII and the traces as in the homogeneous model; the intensity and the PII take the voxel's own rho(v) c(v).  Whether an
 * element is active at a sample is decided in fp64, E_e included (sigma = c_ref / c - 1 stays fp64 on the device).  olx_field_variant
 * then reads "field_pulse_med_k (pulsed through a medium: ... samples, ... planes, R = ...)".  Every reader of the result (scale,
 * aggregate, analysis, olx_pii_post, the thermal sources) sees it exactly as it sees a homogeneous pulsed result.
 * OLX_EINVAL: a uniform absorption (olx_field_absorption > 0), more than 1024 elements (the kernel caches the ray sums of 16 elements
 * per lane), volumes that are not finite / positive.  olx_field_set_medium keeps refusing a pulsed plan: that call selects the
 * continuous-wave kernels. */
int olx_field_pulse_medium(olx_ctx *ctx, const float *sound_speed, const float *attenuation_db_cm_mhz, const float *density,
                           double alpha_power);

/* Thermal model (DESIGN.md section 2 "thermal model", kernel 3): Pennes bioheat rise dT above a baseline over a pulse sequence,
 *   rho Cp d(dT)/dt = div(kappa grad dT) - W dT + Q,   Q = 2 alpha 1e4 I_f(v) while a pulse aimed at focus f is on [W/m^3],
 * explicit FTCS on a grid of its own (7-point stencil, face conductance = harmonic mean of kappa / h^2, dT = 0 one spacing outside the grid).
 * Its buffers are apart from the field / aggregate volumes: a thermal run reads the resident intensity at most and changes nothing of it.
 * Plan the grid and the medium: per-voxel density [kg/m^3], specific heat [J/kg/K], thermal conductivity [W/m/K] and absorption [Np/m]
 * ([nx * ny * nz] floats each, C order), each may be NULL for the uniform value that follows it; perfusion W [W/m^3/K] is uniform.
 * With all four volumes NULL no coefficient volume is formed or streamed.  dt_max_out (may be NULL) receives the FTCS bound
 * 1 / max_v (sum_faces K_face / h^2 + W) / (rho Cp)_v [s] (fp32 coefficients).
 * OLX_EINVAL, before any device call and with a standing thermal plan left as it was: a density, specific heat or conductivity volume
 * holding a value that is not finite and > 0, an absorption volume holding one that is not finite and >= 0 (the message names the
 * volume and the first such voxel); a scalar of a NULL volume that is not > 0 (absorption: not >= 0); perfusion not finite or < 0. */
int olx_thermal_plan(olx_ctx *ctx, const olx_grid *grid, const float *density, const float *specific_heat, const float *conductivity,
                     const float *absorption, double density0, double specific_heat0, double conductivity0, double absorption0,
                     double perfusion, double *dt_max_out);
/* The source schedule of the plan, CSR over n_steps steps: step n heats with sum_e tau[e] s(v) I_{focus[e]}(v), e in
 * [row_ptr[n], row_ptr[n + 1]) (tau = the on-time [s] of the focus' pulses inside the step).  n_points voxels (linear C-order indices)
 * are traced: olx_thermal_fetch returns dT there after every step. */
int olx_thermal_schedule(olx_ctx *ctx, int n_steps, const int *row_ptr, const int *focus, const double *tau, int n_points, const long long *points);
/* The intensity volumes I_f [W/cm^2] the schedule's focus indices refer to: [n_foci * voxels] floats uploaded once, or NULL = the
 * context's resident intensity (a whole-grid result of n_foci foci on the thermal grid, read in place at every olx_thermal_run). */
int olx_thermal_source(olx_ctx *ctx, int n_foci, const float *intensity);
/* Kernel 3 reads the resident PII volumes [J/cm^2] in place as its per-focus source volumes (whole-grid, n_foci foci, on the thermal grid:
 * checked at every olx_thermal_run).  The step kernel is the same: the caller folds 1 / (pulse on-time) into the schedule's tau. */
int olx_thermal_source_pii(olx_ctx *ctx, int n_foci);
/* Steps [first_step, first_step + n_steps) of the schedule with time step dt [s] (<= the FTCS bound) and baseline temperature [deg C];
 * first_step = 0 starts from dT = 0, any other first_step continues the last run.  Per voxel it keeps the maximum rise [K] and
 * CEM43 = sum_n dt / 60 R^(43 - T) [min] (T = baseline + dT after the step, R = 0.5 at T >= 43, 0.25 below).  Asynchronous. */
int olx_thermal_run(olx_ctx *ctx, double dt, double baseline, int first_step, int n_steps);
/* The maximum rise and CEM43 volumes ([voxels] floats) and the traces ([steps run * n_points] floats, step-major); any may be NULL. */
int olx_thermal_fetch(olx_ctx *ctx, float *rise_max, float *cem43, float *traces);

/* Full-wave model (DESIGN.md section 2 "full-wave model", kernel 5): linear acoustics, first order in (p, v), on a staggered grid --
 * second order in time, fourth order in space, fp32 state -- with reflection, refraction and transmission loss at every interface of
 * the medium.  An opt-in model of its own: its buffers are apart from the field plan, the resident result and the thermal buffers, and
 * a full-wave run changes none of them.
 * Plan `grid` -- the PADDED grid: the caller's grid plus pml_size voxels of absorbing layer on every side, the medium extended into the
 * layers by the caller -- and the medium: per-voxel sound speed [m/s], density [kg/m^3] and absorption [Np/m at the drive frequency]
 * ([nx * ny * nz] floats each, C order), each may be NULL for the uniform value that follows; with all three NULL no coefficient volume
 * is formed or streamed.  A layer voxel `depth` voxels into the layer of axis a (1 .. pml_size) decays by
 * exp(-pml_alpha (c_ref / h_a) (depth / pml_size)^4 dt) per step.  dt [s] is the time step of every run of the plan; dt_max_out (may
 * be NULL) receives the stability bound 6 / (7 c_max sqrt(sum_a 1 / h_a^2)).  OLX_EINVAL before the device is touched: dt above the
 * bound, a medium that is not finite and > 0 (absorption >= 0), an axis with no interior voxel, 2^31 voxels or more. */
int olx_fullwave_plan(olx_ctx *ctx, const olx_grid *grid, const float *sound_speed, const float *density, const float *absorption,
                      double sound_speed0, double density0, double absorption0, double c_ref, int pml_size, double pml_alpha,
                      double dt, double *dt_max_out);
/* The source table of the plan: entry s adds amplitude[s] env(u) sin(2 pi freq u), u = (n - 1/2) dt - tau[s], to p at voxels[s]
 * (linear C-order index of the padded grid) at the start of step n while 0 <= u < cycles / freq (decided in fp64); env is 1, or with
 * ramp_cycles > 0 a raised-cosine ramp over the first and the last ramp_cycles / freq seconds.  Entries that share a voxel add in
 * table order.  n_steps is the length of the run (olx_fullwave_run takes steps inside [0, n_steps)); n_points voxels are traced:
 * olx_fullwave_fetch returns p there after every step. */
int olx_fullwave_sources(olx_ctx *ctx, int n_entries, const long long *voxels, const double *amplitude, const double *tau,
                         double freq, double cycles, double ramp_cycles, int n_steps, int n_points, const long long *points);
/* Steps [first_step, first_step + n_steps); first_step = 0 starts from p = v = 0 and clears the records, any other first_step
 * continues the last run (OLX_ESTATE when it does not).  Per voxel it keeps p_max = max_n p and p_min = max_n -p (both >= 0) and,
 * with accumulate_psq != 0, sum_n p^2 (a continued run keeps the choice of its first call).  Asynchronous. */
int olx_fullwave_run(olx_ctx *ctx, int first_step, int n_steps, int accumulate_psq);
/* The records of the padded grid ([voxels] floats each) and the traces ([steps run * n_points] floats, step-major); any may be NULL.
 * OLX_ESTATE: nothing run, or p_sq asked of a run that did not accumulate it. */
int olx_fullwave_fetch(olx_ctx *ctx, float *p_max, float *p_min, float *p_sq, float *traces);
/* Single-frequency lock-in of the run that follows, over the steps n in [first_step, first_step + n_steps):
 * with t_n = (n + 1) dt the time of the recorded p of step n and theta_n = 2 pi frac(freq t_n) formed in double,
 *   volume != 0: per voxel of the padded grid C = sum_n p cosf_n, S = sum_n p sinf_n, one fused multiply-add per step in step order
 *                from 0, with cosf_n / sinf_n the cosine / sine of theta_n rounded once to float;
 *   receiver r < n_receivers: s_r(n) = sum_q weights[q] p(voxels[q]) over q in [row[r], row[r + 1]) in table order, then
 *                C_r += s_r cos theta_n, S_r += s_r sin theta_n, all in double.  An empty row gives 0.
 * Call it after olx_fullwave_sources and before olx_fullwave_run(first_step = 0); a continued run keeps accumulating, and
 * olx_fullwave_sources clears the lock-in.  OLX_EINVAL: a window outside [0, n_steps of the sources), nothing to record, a voxel
 * outside the grid, a row table that does not start at 0 or is not monotone.  OLX_ESTATE: no plan or no sources. */
int olx_fullwave_lockin(olx_ctx *ctx, double freq, int first_step, int n_steps, int volume, int n_receivers, const int *row,
                        const long long *voxels, const double *weights);
/* The lock-in sums: [voxels] floats each, [n_receivers] doubles each; any may be NULL.  OLX_ESTATE: nothing run, something asked
 * for that was not recorded, or the run has not reached the end of the window. */
int olx_fullwave_fetch_lockin(olx_ctx *ctx, float *vol_cos, float *vol_sin, double *rec_cos, double *rec_sin);
/* Finite rectangular element apertures (DESIGN.md section 2 "full-wave model: apertures", section 5.18).  Element e is the rectangle
 * with centre centre[3 e ..] [m, in the frame of the planned grid], in-plane unit axes u_axis[3 e ..] (width) and v_axis[3 e ..]
 * (length) and size size[2 e ..] = (w, l) [m], sampled at the n_w[e] x n_l[e] points
 *   x_ab = c + ((a + 1/2) / n_w - 1/2) w u + ((b + 1/2) / n_l - 1/2) l v,
 * q_ab = (x_ab - origin) / h per axis, a coordinate within 1e-9 of a whole number counting as that number.  The weight of voxel m is
 *   W_e(m) = 1 / (n_w n_l) sum_a sum_b prod_axis max(0, 1 - |q_ab,axis - m_axis|)      (a outer, b inner, double),
 * the trilinear spread of n_w n_l equal monopoles merged per voxel; sum_m W_e(m) = 1.  fullwave_aperture_k evaluates it with one lane
 * per (element, voxel of the element's index box).  Returns a per-element CSR of the weights that are not 0: row[n_el + 1],
 * voxels (linear C-order index of the planned grid, ascending inside a row) and weights.  *n_needed (may be NULL) receives the number
 * of entries; when it is above `capacity` only row is written and the call still returns OLX_OK: call again with room for n_needed.
 * OLX_ESTATE without olx_fullwave_plan.  OLX_EINVAL, naming the element, before any launch: a centre, axis or size that is not finite,
 * a size < 0, n_w or n_l < 1, more than 65536 points, a weighted voxel outside the grid.  Synchronous; changes no source table, run
 * or record. */
int olx_fullwave_apertures(olx_ctx *ctx, int n_el, const double *centre, const double *u_axis, const double *v_axis, const double *size,
                           const int *n_w, const int *n_l, long long capacity, int *row, long long *voxels, double *weights,
                           long long *n_needed);
/* The source table in element-factored form: entry q adds (float)(amplitude[q] s_e(n)), e = elements[q] < n_el, to p at voxels[q] at
 * the start of step n, with the drive s_e(n) = A[e] env(u) sin(2 pi frac(freq u)), u = (n - 1/2) dt - tau[e], exactly 0 outside
 * 0 <= u < cycles / freq (double, as olx_fullwave_sources forms it).  The entries are sorted by voxel, stably, so those of one voxel
 * add in table order; one launch (fullwave_drive_k) fills the drive table s[n_steps][n_el], and each step of olx_fullwave_run then
 * launches fullwave_inject_elem_k in place of fullwave_inject_k.  The other arguments, the reset of the run and of the lock-in are
 * olx_fullwave_sources's, and whichever of the two was called last decides the inject kernel.  OLX_EINVAL before the device is
 * touched: an element outside [0, n_el), a voxel outside the grid, an amplitude, A or tau that is not finite, a drive table above
 * 2^28 bytes (n_steps n_el doubles). */
int olx_fullwave_sources_elements(olx_ctx *ctx, int n_entries, const long long *voxels, const int *elements, const double *amplitude,
                                  int n_el, const double *A, const double *tau, double freq, double cycles, double ramp_cycles,
                                  int n_steps, int n_points, const long long *points);
/* New A[n_el], tau[n_el] for the table of olx_fullwave_sources_elements: re-fills the drive table and resets the run (the next
 * olx_fullwave_run starts at step 0; a lock-in is cleared as by a source call); the entry table stays on the device.  OLX_ESTATE
 * when the last source call was not olx_fullwave_sources_elements. */
int olx_fullwave_drive(olx_ctx *ctx, const double *A, const double *tau);
/* Drives of the element-factored table besides the bare burst (DESIGN.md section 2 "full-wave model: drives", section 5.20).  With
 * s0_e(n) the drive of olx_fullwave_sources_elements, evaluated for negative n too, and g_c[0 .. M_c) the drive taps of element e's
 * class c = class_of_element[e] on the plan's dt grid (taps[row[c] .. row[c + 1])), the drive table becomes
 *   s_e(n) = sum_{m = 0}^{M_c - 1} g_c[m] s0_e(n - m)      (double, m ascending, from 0.0, each product and sum rounded on its own),
 * so taps [1.0] give s0_e(n) bit for bit.  Two launches fill it: fullwave_drive_k evaluates the bare burst for the steps
 * -(M_max - 1) .. n_steps - 1, fullwave_drive_fir_k sums it; the step loop is unchanged.  The argument shape is
 * olx_field_pulse_response's, without its cap on the classes: every element may have its own.  Valid after
 * olx_fullwave_sources_elements; it re-fills the table and resets the run and the lock-in as olx_fullwave_drive does.  n_classes = 0
 * returns to the bare drive (the pointers may be NULL); olx_fullwave_drive (new A, tau) keeps the response; every source call,
 * olx_fullwave_layers and olx_fullwave_plan clear it.  OLX_ESTATE: the last source call was not olx_fullwave_sources_elements, or the
 * table is a sampled one.  OLX_EINVAL before the device is touched: n_classes < 0 or > n_el, a class outside [0, n_classes), a row
 * table that does not start at 0 or is not strictly increasing (a class without taps), more than OLX_PULSE_RESPONSE_MAX_TAPS taps in
 * a class, a tap that is not finite, an extended table ((n_steps + M_max - 1) n_el doubles) above 2^28 bytes. */
int olx_fullwave_drive_response(olx_ctx *ctx, int n_classes, const int32_t *class_of_element, const int32_t *row, const double *taps);
/* Sampled waveforms: table[n_steps][n_el] finite doubles replace the drive table as they are (entry q then adds
 * (float)(amplitude[q] table[n][elements[q]]) at step n).  Same state rule and reset as olx_fullwave_drive_response.  Afterwards
 * olx_fullwave_drive and olx_fullwave_drive_response answer OLX_ESTATE until the next source call: A and tau mean nothing to a sampled
 * table.  OLX_EINVAL, before the device is touched, for a value that is not finite. */
int olx_fullwave_drive_table(olx_ctx *ctx, const double *table);
/* The current drive table, [n_steps][n_el] doubles, as the step loop reads it.  OLX_ESTATE without an element-factored table.
 * Synchronous. */
int olx_fullwave_fetch_drive(olx_ctx *ctx, double *table);
/* The layer model of the plan (DESIGN.md section 2 "full-wave model: split layers", section 5.19): 0 = the multiplicative sponge of
 * olx_fullwave_plan, 1 = split perfectly matched layers.  With sigma_a(d) = pml_alpha (c_ref / h_a) (d / pml_size)^4 of the plan, d_c the
 * depth of a voxel's centre and d_f that of its + face [voxels], r_a = exp(-sigma_a(d_c) dt / 2) and s_a = exp(-sigma_a(d_f) dt / 2)
 * (double, rounded once to float), the split model steps v_a <- s_a (s_a v_a - b_a d+_a p) in every voxel and, in a layer voxel
 * (d_c > 0 on any axis), three components p_a <- ga (r_a (r_a p_a - (kp d-_a v_a) / h_a)) with p = (p_x + p_y) + p_z; interior voxels
 * and every record are the sponge's with D = 1.  Sources must then lie on interior voxels: the source calls answer OLX_EINVAL for an
 * entry on a layer voxel.  Call it after olx_fullwave_plan; it clears the sources, the lock-in and the run as a source call does, and
 * every olx_fullwave_plan returns to the sponge.  The first split model creates three more [voxels] float volumes.  OLX_ESTATE without
 * a plan, OLX_EINVAL for any other model. */
int olx_fullwave_layers(olx_ctx *ctx, int model);

/* Eikonal travel times (DESIGN.md section 2 "Eikonal", kernel 6): first-arrival times T [s] from the point source_m through the sound
 * speed of `grid` ([nx * ny * nz] floats, C order; NULL = c_uniform everywhere, and no volume is streamed), refraction included.
 * Voxels within init_radius voxels of the source (index space) start at |x_v - x_t| / c(v) and stay; the others are lowered by Jacobi
 * sweeps of the first-order upwind update (fp32 state) until a sweep changes no voxel.  *sweeps_out (may be NULL) = the number of
 * sweeps, that last one included.  Synchronous.  Buffers of its own: the plan, the resident result, the thermal and the full-wave
 * buffers stay as they are.  OLX_EINVAL before the device is touched: a speed that is not finite and > 0, a source outside
 * [0, n_a - 1] index coordinates on an axis, init_radius < 1, max_sweeps < 1, 2^31 voxels or more.  OLX_ENOCONV when max_sweeps
 * sweeps did not converge: no field is kept (olx_eikonal_sample / _fetch then return OLX_ESTATE), the context stays usable. */
int olx_eikonal_solve(olx_ctx *ctx, const olx_grid *grid, const float *sound_speed, double c_uniform, const double *source_m,
                      double init_radius, int max_sweeps, int *sweeps_out);
/* T of the last solve at n_points points: t_out[r] = sum_q weights[q] (double) T(voxels[q]) over q in [row[r], row[r + 1]) in table
 * order, in double.  OLX_ESTATE before a converged solve.  OLX_EINVAL: n_points < 1, a voxel outside the grid, a weight that is not
 * finite, a row table that does not start at 0 or is not monotone.  Synchronous. */
int olx_eikonal_sample(olx_ctx *ctx, int n_points, const int *row, const long long *voxels, const double *weights, double *t_out);
/* The whole volume of the last solve ([voxels] floats, +inf where nothing arrived).  OLX_ESTATE before a converged solve. */
int olx_eikonal_fetch(olx_ctx *ctx, float *t_out);

/* ---- kernel 4: steering map (DESIGN.md section 2 "Steering map") ---------------------------------------
 * Where can the array steer?  Every voxel of `grid` is a candidate target, in the frame of the element table (kernel 1 with
 * M = identity): with w = r_v - g_e, d = |w|, d' = max(d, min(spacing) / 2) and theta = kernel 1's folded angle,
 *   pfocal_out[v]   = (p0_pa / lambda) sum_e a_e S_e D_e(v) exp(-absorption d') / d'   [Pa]
 *   n_active_out[v] = #{ e : a_e > 0 }
 * a_e = the apodization of olx_bf_solve (apod_kind, p0, p1; OLX_APOD_RADIANS honoured), S_e = area_m2 of olx_set_elements, D_e = the
 * piston factor of olx_set_element_apertures with flags = OLX_FIELD_DIRECTIVITY (1 with flags = 0), absorption_np_m >= 0 a uniform
 * absorption.  pfocal is the CW |p| of olx_field_* at v when the array is steered to v with untruncated Direct delays and this
 * apodization.  fp32 results within 1e-5 of the volume maximum; the a_e > 0 decisions are made in fp64.
 * Uses the resident element table (OLX_ESTATE without one, or without apertures when directivity is flagged).  Both volumes
 * ([nx*ny*nz], C order; n_active_out may be NULL) are buffers of the context's own, created by the first call and reused: the
 * current plan, the steering table and every resident result are left untouched.  Synchronous. */
int olx_steer_map(olx_ctx *ctx, const olx_grid *grid, double freq, double c, double p0_pa,
                  int apod_kind, double p0, double p1, double absorption_np_m,
                  unsigned flags /* 0 | OLX_FIELD_DIRECTIVITY */,
                  float *pfocal_out, int *n_active_out /* may be NULL */);
/* Times `iters` repeats of the last olx_steer_map's map kernel (same grid and options, results rewritten with equal values) with
 * HIP events on the context's stream; ms_each[iters] = milliseconds per launch (tools/time_steer.py).  OLX_ESTATE before a map. */
int olx_steer_time(olx_ctx *ctx, int iters, float *ms_each);

/* ---- kernel 4h: steering map through a heterogeneous medium, straight rays (DESIGN.md section 2 "Steering map through a medium") ----
 * olx_steer_map with the medium on every ray.  The volumes (float32 [nx*ny*nz] on `grid`, C order; NULL = c_ref everywhere / no
 * attenuation) are sound speed [m/s] and attenuation [dB/cm/MHz^0.9], converted at `freq` as olx_bf_set_attenuation does.  With w, d, d',
 * theta, b_e = the base apodization (apod_kind, p0, p1), S_e, D_e and n_active exactly as olx_steer_map's, voxel v = (i, j, kv):
 *   K_e(v) = the grid planes k != kv strictly between z_e and z_v (kernel 2h's plane bounds, decided on the host in fp64)
 *   A_e    = 0 if z_v == z_e, else l (a(v) / 2 + sum_{k in K} a_k(crossing_k)),  l = hz d' / |z_v - z_e|,   E_e = the same over c_ref / c - 1
 *   h_e    = exp(-A_e)  [S_e / d' with spreading]
 *   c_e    = b_e (OLX_STEER_COMP_NONE) | b_e min_active h / h_e (OLX_COMP_EQUALIZE) | b_e h_e / max_active h (OLX_COMP_MATCHED), active = { b_e > 0 };
 *            no active element: 0
 *   pfocal_out[v] = (p0_pa / lambda) sum_e c_e S_e D_e exp(-A_e) / d'                                   (OLX_STEER_DELAYS_STRAIGHTRAY)
 *                 = (p0_pa / lambda) | sum_e c_e S_e D_e exp(-A_e) / d' exp(j 2 pi E_e / lambda) |      (OLX_STEER_DELAYS_DIRECT), lambda = c_ref / freq
 * At a grid voxel A_e and E_e are kernel 1a's and 1m's ray sums with the focus at r_v, so pfocal is the |p| at v of the sampled
 * heterogeneous field (olx_field_set_medium, OLX_MEDIUM_SAMPLED, one plane per layer) when the array is steered to v with
 * olx_bf_solve_compensated / olx_bf_solve_medium (StraightRay) or olx_bf_solve (Direct).  With both volumes NULL it is olx_steer_map's map
 * with absorption 0.  fp32 results within 1e-5 of the volume maximum; the b_e > 0 decisions are made in fp64.  An h_e that underflows is
 * outside the method's range.
 * Refused like olx_steer_map (no elements; directivity without apertures; a bad grid; freq / c_ref not finite and > 0), and for a sound
 * speed <= 0 or non-finite, an attenuation negative or non-finite, an unknown comp / delays; a refusal touches nothing on the device.
 * The stencil, the plane lists, the element records and both result volumes are buffers of the context's own, created by the first call
 * and reused: the plan and its medium, the steering table, the media of olx_bf_set_medium / olx_bf_set_attenuation and every resident
 * result are left untouched.  Synchronous; olx_steer_time repeats the last map of either kind. */
#define OLX_STEER_COMP_NONE (-1)
enum { OLX_STEER_DELAYS_STRAIGHTRAY = 0, OLX_STEER_DELAYS_DIRECT = 1 };
int olx_steer_map_medium(olx_ctx *ctx, const olx_grid *grid, double freq, double c_ref, double p0_pa,
                         int apod_kind, double p0, double p1,
                         const float *sound_speed /* [nx*ny*nz] or NULL = c_ref */,
                         const float *attenuation_db_cm_mhz /* or NULL = none */,
                         int comp /* OLX_STEER_COMP_NONE | OLX_COMP_EQUALIZE | OLX_COMP_MATCHED */, int spreading,
                         int delays /* OLX_STEER_DELAYS_STRAIGHTRAY | OLX_STEER_DELAYS_DIRECT */,
                         unsigned flags /* 0 | OLX_FIELD_DIRECTIVITY */, float *pfocal_out, int *n_active_out /* may be NULL */);

/* Bind host volumes (e.g. a Solution loaded from disk) as the context's resident result so
 * that the aggregate / scale / masked-peak entry points can run on them: [n_foci * slab voxels]
 * floats each; intensity may be NULL.  Needs no element or steering table; olx_field_launch is
 * refused afterwards until the next olx_field_plan.  Like a plan it resets olx_field_aggregate_counts
 * (aggregates cover all n_foci uploaded volumes) and drops any heterogeneous-medium state. */
int olx_field_upload(olx_ctx *ctx, const olx_grid *grid, const olx_slab *slab, int n_foci,
                     const float *pmag, const float *intensity);

/* Times `iters` back-to-back launches with HIP events on the context's stream
 * (bench.py roofline leg); ms_each[iters] receives per-launch milliseconds. */
int olx_field_time(olx_ctx *ctx, int iters, float *ms_each);
/* In-stream kernel timing for bench.py: between begin and end every olx_field_launch is bracketed
 * by a pair of HIP events recorded on the context's stream (the stream the kernel runs on), up to
 * max_launches.  end synchronises the stream and returns the per-launch kernel durations [ms]. */
int olx_profile_begin(olx_ctx *ctx, int max_launches);
int olx_profile_end(olx_ctx *ctx, float *ms_each, int capacity, int *n_recorded);

/* Times one of the HBM-bound streaming scans over the resident result (bench.py: GB/s against the roofline): `iters`
 * back-to-back launches on the context's stream, HIP events between them; *bytes_per_launch = algorithmic bytes of one launch
 * (F = planned foci, V = slab voxels): aggregate V (8 F + 8), scale 16 F V (by 1.0: the result is unchanged), the six-peak
 * analysis scan 8 F V, one masked |p| peak 4 F V, the fp64 offset grid 32 V (coords + distance, written to scratch), the
 * weighted intensity sum V (4 F + 4).  Needs a plan with intensity output. */
#define OLX_SCAN_AGGREGATE 0
#define OLX_SCAN_SCALE 1
#define OLX_SCAN_ANALYSIS_PEAKS 2
#define OLX_SCAN_MASKED_PEAK 3
#define OLX_SCAN_OFFSET_GRID 4
#define OLX_SCAN_WEIGHTED_SUM 5
#define OLX_SCAN_FUSED_POST 6   /* scale + aggregate + six peaks + time-average volume in ONE pass (<= 8 foci): V (16 F + 12) bytes */
#define OLX_SCAN_PII_SCALE 7    /* olx_pii_post over the resident PII (not the planned volumes), factors only: V (8 F + 4) bytes -- 4 more than the scaling
                                 * alone needs, on purpose: every form stores max_f PII_f, so olx_pii_fetch_max is current after every scaling */
#define OLX_SCAN_PII_FULL 8     /* ... factors, weights and peaks: V (8 F + 8) bytes */
int olx_scan_time(olx_ctx *ctx, int kernel, int iters, float *ms_each, double *bytes_per_launch);

/* Name of the field kernel variant the current plan dispatches to (for profiles and tests).  A launch of kernel 2m (OLX_MEDIUM_MARCHED) appends the
 * launch sequence it ran, rebuilt by every launch: "; 2m: inside|border, lookup0 xN, writer0 x1, lookup xN, writer xN, texel xN" -- inside: every
 * element at least half a cell inside the lateral grid (no clamp of the look-up coordinates), else border; lookup0 / writer0: look-up launches below
 * and the writer of the first non-trivial plane (no source sums); lookup / writer: those that read running sums; texel: the one-sum look-ups above
 * the medium out of the row-pair form; kinds that did not run are left out -- and then, with OLX_MARCH_FUSE, "; fused writers: P planes in L launches". */
const char *olx_field_variant(const olx_ctx *ctx);

/* ---- aggregation over foci (plan/protocol.py:382-387) ------------------------------
 * p_agg = max_f |p_f|, I_agg = mean_f I_f over the planned volumes, on device;
 * host outputs [slab voxels], either may be NULL. */
int olx_field_aggregate(olx_ctx *ctx, float *pmag_max_out, float *intensity_mean_out);
/* The same aggregate left in HBM (nothing copied): olx_aggregate_fetch brings either volume to the host when -- and if --
 * the caller reads it (Protocol.calc_solution hands the aggregate Dataset out lazily, like the per-focus volumes).
 * The buffers are reused by the next aggregate and freed by a plan / upload that needs larger volumes. */
int olx_field_aggregate_device(olx_ctx *ctx, int want_intensity);

/* Per-focus in-place scaling (plan/solution.py:331-337): p_f *= s_f, I_f *= s_f^2. */
int olx_field_scale(olx_ctx *ctx, const double *scale_per_focus, int n_foci);
/* olx_field_scale followed by olx_field_aggregate_device(ctx, 1) in one pass over the volumes (the two steps
 * Protocol.calc_solution(scale=True) runs back to back, plan/protocol.py:374-387): identical values, the volumes cross HBM
 * twice instead of three times.  Needs intensity output. */
int olx_field_scale_aggregate(olx_ctx *ctx, const double *scale_per_focus, int n_foci);

/* Per-focus masked peak (plan/solution_analysis.py:384-442 get_mask, consumed by
 * Solution.analyze, plan/solution.py:205-262).  For focus f and voxel position r [m]:
 *   q = A_f . [r, 1]   (A_f = first three rows of inv(get_focus_matrix(focus_f, origin_f)),
 *                       solution_analysis.py:319-342; row-major, A[F*12])
 *   dist = sqrt(sum_a (q_a / aspect[a])^2)
 * the voxel is selected when `dist OP radius_m` (op 0 '<', 1 '<=', 2 '>', 3 '>=', 4 = no
 * distance test) and, if use_zmin, its z coordinate > zmin_m.  peak_out[F] receives the max
 * over selected voxels of |p_f| (which = 0), intensity_f (which = 1) or the single weighted-intensity
 * volume of olx_field_weighted_intensity (which = 2); 0 when none selected. */
int olx_field_masked_peak(olx_ctx *ctx, int which, const double *A, const double *aspect,
                          double radius_m, int op, int use_zmin, double zmin_m, float *peak_out);

/* The six peaks Solution.analyze takes from |p_f| and intensity_f (plan/solution.py:205-262) in one pass over both volumes:
 * peaks_out[F*6] = per focus (mainlobe |p|, mainlobe I, sidelobe |p|, sidelobe I, global |p|, global I) with
 * mainlobe = dist < r_main_m, sidelobe = dist > r_side_m and z > zmin_m, global = z > zmin_m -- the same arithmetic as six
 * olx_field_masked_peak calls (ops '<', '>' and none), bit-identical results, one sixth of the HBM reads and launches. */
int olx_field_analysis_peaks(olx_ctx *ctx, const double *A, const double *aspect, double r_main_m, double r_side_m,
                             double zmin_m, float *peaks_out);

/* Masked first moments per focus (find_centroid, plan/solution_analysis.py:306-317): over voxels with
 * dist < radius_m (same focal-ellipsoid metric as above) and |p_f| > cutoff[f]:
 * moments_out[F*4] = { sum p, sum p x, sum p y, sum p z } (x, y, z = voxel position in metres, fp64). */
int olx_field_masked_moments(olx_ctx *ctx, const double *A, const double *aspect, double radius_m,
                             const float *cutoff, double *moments_out);

/* Trilinear samples of focus volume `focus` (|p| for which = 0, intensity for which = 1) at npts points
 * pts_m[npts*3] (metres); NaN outside the grid, like the xarray interpolation behind get_beamwidth
 * (plan/solution_analysis.py:444-574). */
int olx_field_sample(olx_ctx *ctx, int which, int focus, const double *pts_m, int npts, float *out);

/* Offset grid of ANY coordinate grid (get_gridded_transformed_coords / get_offset_grid / calc_dist_from_focus,
 * plan/solution_analysis.py:344-403): the grid is given by its three axis vectors xs[nx], ys[ny], zs[nz] (the
 * DataArray coords, any units); A[12] = first three rows of inv(get_focus_matrix(focus, origin)), row-major.
 * coords_out[nx*ny*nz*3] (C order, last axis = d_x, d_y, d_z) and / or dist_out[nx*ny*nz] =
 * sqrt(sum_a (coords_a / aspect[a])^2) (aspect NULL = [1,1,1]); fp64, same operation order as the reference's
 * np.dot rows.  Needs no element table or plan. */
int olx_offset_grid(olx_ctx *ctx, const double *xs, int nx, const double *ys, int ny, const double *zs, int nz,
                    const double *A, const double *aspect, double *coords_out, double *dist_out);

/* Time-of-flight spread over a grid (SimSetup.get_max_cycle_offset, sim/sim_setup.py:132-143): for every grid
 * point (axis vectors in metres) tof_e = dist(point, element e) / c0 + delays_s[e] (NULL = zeros) over the resident
 * element table; *max_dtof_s = max over points of (max_e tof - min_e tof), fp64.  The caller multiplies by the
 * frequency and applies the zmin cut by passing the z axis it wants. */
int olx_tof_spread(olx_ctx *ctx, const double *xs, int nx, const double *ys, int ny, const double *zs, int nz,
                   const double *delays_s, double c0, double *max_dtof_s);

/* out[v] = max_f weights[f] * intensity_f[v] kept on the device as the "time-average" volume of Solution.analyze.
 * Why a maximum: the reference's get_ita (plan/solution.py:365-388) multiplies its [focal_point_index, x, y, z] intensity,
 * expanded on the LAST axis, with pulse counts shaped [1, 1, 1, F] -- the counts cancel, every focus volume is its own
 * intensity times the two duty cycles -- and analyze takes `.where(mask).max()` / `(ita * z_mask).max()` over that whole
 * stack (plan/solution.py:243, 274), i.e. the maximum over foci AND voxels.  olx_field_masked_peak(which = 2) scans THIS
 * single volume with every focus' mask and so returns the reference's numbers.  (Rounds 1-4 formed sum_f here.) */
int olx_field_weighted_intensity(olx_ctx *ctx, const double *weights, int n_foci);
/* Blocking copy of that volume ([slab voxels] floats) into a caller-owned array: max_f w_f I_f, the ONE volume analyze's masked
 * maxima scan.  (Solution.get_ita itself returns the whole [focal_point_index, x, y, z] stack, plan/solution.py:365-388; the host
 * mirror forms it from the per-focus intensities, not from this volume.)  The volume is the one the last
 * olx_field_weighted_intensity or olx_solution_analyze left on the device.
 * ABI note: with OLX_ABI_VERSION 2 the reduction over foci of olx_field_weighted_intensity changed from SUM to MAX (see above);
 * a caller built against ABI v1 gets different numbers for F > 1 -- check olx_abi_version(). */
int olx_field_weighted_fetch(olx_ctx *ctx, float *out);

/* ---- one-call analysis (Solution.analyze, plan/solution.py:135-281) ---------------------
 * Everything analyze() reads off the resident volumes in ONE crossing: the six masked peaks of olx_field_analysis_peaks,
 * the -3 dB centroid moments (olx_field_masked_moments with cut-off = mainlobe |p| peak * centroid_factor, fp32 product),
 * the time-average volume of olx_field_weighted_intensity with its per-focus mainlobe peaks and its global peak above
 * zmin (*ita_global), and the beam-width crossings of get_beam_bounds (solution_analysis.py:488-535) along the three focal
 * axes.  Same kernels and arithmetic as the separate entry points (results identical); no intermediate leaves the device.
 *   A[F*12]            focal frames as for olx_field_masked_peak
 *   ita_weights[F]     per-focus weights of the time-average intensity
 *   line_pts           [F][n_line[0] + n_line[1] + n_line[2]][3] sample positions [m] of each focus' lateral, elevation and
 *                      axial line (the caller forms them: offsets linspace(-r, r, n) mapped through its focus matrix);
 *                      may be NULL when all n_line are 0 (no beam widths; bounds = -1)
 *   n_le[a] / i_ge[a]  number of leading samples of line a whose offset is <= 0 / index of its first sample with offset >= 0
 *   beam_factor[2]     cut-off of level l = (float)(mainlobe |p| peak * beam_factor[l])  (10^(-3/20), 10^(-6/20))
 *   scale_per_focus    NULL: the volumes as they are.  [F] factors: olx_field_scale_aggregate happens FIRST (Solution.scale +
 *                      the aggregation, plan/protocol.py:374-387; olx_aggregate_fetch reads the aggregate afterwards) and the
 *                      analysis sees the scaled volumes -- for <= 8 foci in ONE pass over the volumes together with the peak
 *                      scan and the time-average volume (the values of the separate calls)
 * bounds[a][l][0] = index within line a of the LAST sample at an offset <= 0 below the cut-off, [1] = the FIRST at an offset
 * >= 0; -1 = none (NaN samples -- outside the grid -- never qualify). */
typedef struct olx_analysis_opts {
    double aspect[3];
    double r_main_m, r_side_m, zmin_m;
    double beam_factor[2];
    float centroid_factor;
    int32_t n_line[3], n_le[3], i_ge[3];
} olx_analysis_opts;
typedef struct olx_focus_report {
    float peaks[6];          /* mainlobe |p|, mainlobe I, sidelobe |p|, sidelobe I, global |p|, global I */
    float ita_main;          /* mainlobe peak of the time-average intensity volume */
    float reserved;
    double moments[4];       /* S0 = sum |p|, S1 = sum |p| (x, y, z) [m] over the -3 dB mainlobe voxels */
    int32_t bounds[3][2][2];
} olx_focus_report;
int olx_solution_analyze(olx_ctx *ctx, const double *A, const double *ita_weights, const double *line_pts,
                         const olx_analysis_opts *opts, const double *scale_per_focus, olx_focus_report *reports,
                         float *ita_global);
/* The same in two halves, for callers that have host work of their own to do meanwhile (Solution.analyze evaluates the emitted pressure / power /
 * thermal index beside it): _begin copies its arguments, enqueues every kernel and the copy of the report on the context's stream and returns;
 * _finish waits for the stream and unpacks the report.  Between the two the context must not be used for anything else (one caller thread per
 * context; every other entry point that touches the stream would order itself behind the analysis anyway).  olx_solution_analyze = both. */
int olx_solution_analyze_begin(olx_ctx *ctx, const double *A, const double *ita_weights, const double *line_pts,
                               const olx_analysis_opts *opts, const double *scale_per_focus);
int olx_solution_analyze_finish(olx_ctx *ctx, olx_focus_report *reports, float *ita_global);

/* ---- multi-GPU reassembly (RCCL over xGMI) -------------------------------------------
 * One context per rank.  id_bytes = the 128-byte ncclUniqueId made by rank 0
 * (olx_comm_unique_id) and distributed by the host launcher.  olx_field_allgather
 * gathers every rank's planned |p| block (n_foci * slab voxels floats, equal on all
 * ranks) into a device buffer of nranks blocks in rank order, asynchronously on a
 * side stream ordered after the last olx_field_launch; olx_allgather_fetch copies
 * rank r's block to the host. */
#define OLX_UNIQUE_ID_BYTES 128
/* Transport (environment OLX_GATHER, read by rank 0 in olx_comm_unique_id; the id tells the other ranks):
 *   rccl (default)  ncclAllGather / all-reduce / reduce-scatter over RCCL;
 *   p2p             direct all-gather without RCCL: every rank PULLS each peer's block over its own xGMI link, all links at
 *                   once, out of output buffers mapped with HIP IPC (works for ranks that share one device too).  The output
 *                   blocks are reallocated by olx_field_plan, so after EVERY plan each rank calls olx_comm_export
 *                   (OLX_P2P_BLOB_BYTES), the launcher all-gathers the blobs in rank order and each rank calls olx_comm_import
 *                   with all of them.  The aggregate exchanges take the same road: rank r owns slice r of the volume, pulls
 *                   that slice of every peer's partial, reduces in rank order (same bits on every rank) and -- all-reduce --
 *                   the ranks pull each other's reduced slices.
 * olx_comm_transport names what this context uses ("rccl", "p2p", "" before olx_comm_init).
 * Lifetime rules of the p2p transport: a rank's output and aggregate blocks are mapped by its peers, so every call that frees or
 * rewrites them in place (a larger olx_field_plan, olx_field_upload, olx_field_scale*, the fused olx_solution_analyze,
 * olx_comm_destroy / olx_ctx_destroy) first waits until every peer has finished the pulls it owes.  Any wait gives up after
 * OLX_P2P_TIMEOUT_S seconds (default 60) and raises an abort flag shared by all ranks: after ANY call has returned OLX_ECOMM the
 * communicator is dead on every rank -- olx_comm_destroy it and build a new one (olx_comm_unique_id / olx_comm_init); the context,
 * its plan and its resident volumes stay usable.
 * olx_comm_ranks_seen = the number of ranks the transport itself has counted (ncclCommCount; ranks attached to the p2p control
 * block), 0 without a communicator -- what a launcher prints to prove how many ranks really met. */
#define OLX_P2P_BLOB_BYTES 384
int olx_comm_ranks_seen(olx_ctx *ctx);
int olx_comm_export(olx_ctx *ctx, void *blob_out);
int olx_comm_import(olx_ctx *ctx, const void *blobs);
const char *olx_comm_transport(const olx_ctx *ctx);
int olx_comm_unique_id(olx_ctx *ctx, void *id_bytes);
int olx_comm_init(olx_ctx *ctx, const void *id_bytes, int nranks, int rank);
int olx_comm_destroy(olx_ctx *ctx);
int olx_field_allgather(olx_ctx *ctx);
int olx_allgather_fetch(olx_ctx *ctx, int rank, float *pmag_out);
/* Aggregated result with the foci sharded over ranks (plan/protocol.py:382-387): local max / sum over
 * this rank's foci, then RCCL all-reduce (max for |p|, sum for the intensity mean) of one volume each,
 * asynchronously on the side stream; the mean divides by n_foci * nranks (equal foci per rank) unless
 * olx_field_aggregate_counts gave the genuine counts of padded shards.
 * olx_field_reduce_scatter_aggregate is the sharded form: an in-place reduce-scatter after which rank r owns voxels
 * [r V/N, (r+1) V/N) of the global aggregate (the rest of its buffer holds its local partial result) -- half the
 * xGMI traffic; it falls back to the all-reduce when V is not divisible by N.
 * olx_aggregate_fetch waits for either and copies the volumes to the host (either may be NULL). */
int olx_field_allreduce_aggregate(olx_ctx *ctx);
int olx_field_reduce_scatter_aggregate(olx_ctx *ctx);
/* Shards padded to equal size (RCCL all-gather needs equal counts; dist.plan_foci_orbits repeats a rank's last focus):
 * only the first local_valid planned foci of this rank enter its local max / sum, and the intensity mean divides by
 * global_total (the number of genuine foci over all ranks).  Valid until the next olx_field_plan / olx_field_upload. */
int olx_field_aggregate_counts(olx_ctx *ctx, int local_valid, int global_total);
/* File the RCCL entry points were bound from ("" before the first olx_comm_* call). */
const char *olx_rccl_path(const olx_ctx *ctx);
int olx_aggregate_fetch(olx_ctx *ctx, float *pmag_max_out, float *intensity_mean_out);

#ifdef __cplusplus
}
#endif
#endif /* OLX_H */
