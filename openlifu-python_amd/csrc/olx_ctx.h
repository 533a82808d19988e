// Host-side context of the C-ABI (include/olx.h): device buffers, plan state, variant decisions.
// Shared by olx.hip and the kernel translation units' launchers.
#pragma once
#include "../../include/olx.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "olx_params.h"
#include "olx_plan.h"

using namespace olx;

// ---- RCCL, bound at run time so that single-GPU use never loads it -------------------
typedef struct { char internal[OLX_UNIQUE_ID_BYTES]; } olx_nccl_id;
typedef void* olx_nccl_comm;
struct RcclApi {
    void* handle = nullptr;
    int (*GetUniqueId)(olx_nccl_id*) = nullptr;
    int (*CommInitRank)(olx_nccl_comm*, int, olx_nccl_id, int) = nullptr;
    int (*CommDestroy)(olx_nccl_comm) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int /*dtype*/, olx_nccl_comm, hipStream_t) = nullptr;
    int (*AllReduce)(const void*, void*, size_t, int /*dtype*/, int /*op*/, olx_nccl_comm, hipStream_t) = nullptr;
    int (*ReduceScatter)(const void*, void*, size_t /*recvcount*/, int /*dtype*/, int /*op*/, olx_nccl_comm, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    int (*CommCount)(olx_nccl_comm, int*) = nullptr;
};
static constexpr int kNcclFloat32 = 7;  // ncclFloat32 in rccl.h's ncclDataType_t
static constexpr int kNcclSum = 0, kNcclMax = 2;  // ncclRedOp_t

struct olx_ctx;

// A device buffer of n elements of T: owned (freed with its owner), never copied -- passing one by value, through a templated launch
// wrapper say, fails to compile instead of freeing the block twice.  Reads as a T* (kernel arguments, offsets, null tests).
template <class T> class DevBuf {
    T* p = nullptr;
    size_t cap = 0;     // elements
public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    int reserve(olx_ctx* c, size_t n);     // room for n elements (at least one); grows only, and a block that grows does not keep its contents
    void release() { if (p) hipFree(p); p = nullptr; cap = 0; }
    size_t capacity() const { return cap; }
    operator T*() const { return p; }
};

struct FetchLane;   // olx.hip: pinned staging of the device -> host fetches
struct P2PState;    // olx_p2p.hip: direct peer-to-peer reassembly (OLX_GATHER=p2p)

struct olx_ctx {
    int device = 0;
    FetchLane* fetch_lanes = nullptr;          // per context, created on the first staged fetch
    bool near = false;                         // a voxel comes within a quarter wavelength of an element: kernels 2a / 2b / 2c take their coordinates as (index, residual)
    bool tab_split = false;                    // kernel 2a's table holds such coordinates (near, or the modifier kernel)
    int n_cu = 0;                              // compute units of the device (persistent kernels size their grids by it)
    hipStream_t stream = nullptr;
    std::string err;
    // element table (device fp64 SoA + host copy for variant decisions)
    int n_el = 0;
    DevBuf<double> d_pos, d_nrm, d_area;
    std::vector<double> h_pos;  // [3][N]
    std::vector<double> h_area, h_delays, h_apod;  // host mirrors for variant decisions
    std::vector<double> h_foci; unsigned long long foci_version = ~0ull;  // foci of the last olx_bf_solve in the element frame (M == identity)
    // optional piston directivity: local x axes [N][3] and sizes [N][2] on the host, packed frame table on the device
    std::vector<double> h_xaxis, h_size, h_nrm; DevBuf<float> d_tab2; bool directivity = false; double absorb_np_m = 0;   // per-term factors beyond w / d: piston directivity, uniform absorption (the live setting, "for the plans that follow")
    double plan_absorb = 0;     // olx_field_absorption as seen by the last olx_field_plan: what that plan's launches carry, whatever the setting became since
    bool modifier() const { return directivity || plan_absorb > 0; }      // of the PLAN (olx_field_plan sets both before it asks)
    bool dir_lattice = false;   // dir_lattice: flat, axis-aligned, equal-size elements -> D_e folds into the lattice kernels' tables
    bool allow_shared = true;
    // steering
    int n_foci = 0;
    DevBuf<double> d_delays, d_apod, d_foci, d_M;
    unsigned long long steer_version = 0, packed_version = ~0ull, configured_version = ~0ull;   // steering table / what the operands were packed from / what configure_variant decided for
    // field plan
    bool planned = false;
    std::string plan_env;   // OLX_FIELD_VARIANT | OLX_FP8_CORRECTION as seen by the last olx_field_plan (a changed pin forces a full re-plan)
    bool uploaded = false;  // volumes came from olx_field_upload: not launchable
    olx_grid grid{};
    olx_slab slab{};
    int plan_foci = 0;
    double freq = 0, c = 0, rho = 0, p0_pa = 0;
    unsigned flags = 0;
    FieldParams fp{};
    bool flat = false, clamp = false;
    // shared-geometry variant (kernel 2b): mirror folds and foci per tile; 1,1,1 = kernel 2a
    bool use_mfma = false; int nt = 1; MfmaParams mp{}; DevBuf<float4> d_coords; DevBuf<uint4> d_bfrag; DevBuf<int> d_colinfo;
    int* d_targets = nullptr;                  // (not owned) the store targets: the tail of d_colinfo
    double min_dist = 0, mfma_wscale = 0; int force_kind = 0;  // 0 auto, 1 general, 2 shared, 3 mfma
    int mx = 1, my = 1, dx = 1, dy = 1, nf = 1; std::vector<int> h_px, h_py; DevBuf<int> d_perm; SharedParams sp{};
    DevBuf<float> d_tab;
    // lattice variant (kernel 2d): matrix array whose pitch is a whole number of voxels
    typedef olxplan::Lattice Lattice;          // olx_plan.h: regular (a, b) lattice in one z plane, pitch = whole voxels
    Lattice lat;
    bool use_lattice = false; int lat_mt = 8; LatParams lp{}; DevBuf<int> d_slot;
    std::vector<double> nf_s2;   // [plane block q]: max_v sum_e 1 / d'(v, e)^2 over the planes >= 16 q of the planned slab [1/m^2] (olxplan::nearfield_s2; < 0 = not derived yet): the e4m3 error bound's near-field term
    int fp8_kcut = 0;            // e4m3 correction products for the plane blocks from this plane on, fp16 x 3 below (0: everywhere); meaningful while fp8corr
    unsigned cp_nfar = 0;        // block records [0, cp_nfar): planes >= fp8_kcut; [cp_nfar, cp_nblocks): the planes below (their operands sit bfrag_half / afrag_half further on)
    size_t bfrag_half = 0, afrag_half = 0;
    bool use_coset = false; bool fp8corr = false; CosetParams cp{}; DevBuf<int> d_jobs;   // kernel 2e (whole cosets per wave) instead of 2d's row tiles
    // kernel 2f (one steering column: Toeplitz weights stationary, 16 planes per MFMA tile)
    DevBuf<CosetBlock> d_cpblocks; unsigned cp_nblocks = 0;   // kernel 2g block records
    int up_blocks_key[17] = {0};              // the partition up_blocks was derived from
    std::vector<CosetBlock> up_blocks; std::vector<int> up_jobs, up_slot;   // host copies of what d_cpblocks / d_jobs / d_slot hold (re-uploaded only when they change)
    std::vector<int> up_perm, up_colinfo;                                  // ... and of d_perm / d_colinfo (a new target of the same pattern changes none of them)
    bool use_cosetp = false;   // kernel 2g: 2e's NT = 2 shape with the planes in the MFMA rows (no output staging)
    bool use_toep = false; int toep_nsa = 0, toep_saw = 16; unsigned toep_ksmask = 0; int toep_nm = 1;   /* row tiles per block (ToepShape) */   /* super-block columns, their width, non-zero K-steps */ int toep_targets[4] = {-1, -1, -1, -1};
    DevBuf<int> d_cell; DevBuf<uint4> d_afrag;
    static constexpr int NBUF = 2;
    DevBuf<float> d_pmag[NBUF];               // the output volumes (reserve_outputs): |p| ...
    DevBuf<float> d_inten, d_cplx, d_agg_p, d_agg_i;   // ... and the members created lazily at its capacity
    // Intensity of a launched continuous-wave plan in a homogeneous medium: DERIVED -- no kernel 2 variant stores it, d_inten is not reserved, and every
    // reader forms olx_inten(|p|, fp.inten_scale) from the |p| volumes (k_types.hip.h).  Pulsed plans, heterogeneous media, uploaded results and plans
    // made under OLX_INTENSITY_STORED=1 keep the stored volumes.  `flags` keeps OLX_OUT_INTENSITY either way; the kernels' own flags drop the bit.
    bool derive_i = false;
    bool inten_live = false;                  // derive_i: d_inten holds olx_inten of the |p| volumes as they are now (materialize_intensity; a launch, a scaling or a plan ends it)
    DevBuf<float> d_ifetch;                   // derive_i: one volume of scratch the intensity fetches fill focus by focus (created by the first of them)
    DevBuf<float> d_scale;
    DevBuf<double> d_peakA; DevBuf<unsigned> d_peak;
    DevBuf<float> d_wint;  // weighted-intensity (time-average) volume
    DevBuf<unsigned char> d_an; void* h_an = nullptr; size_t h_an_bytes = 0;   // olx_solution_analyze: device scratch, pinned staging
    bool an_pending = false; int an_F = 0, an_npts = 0; size_t an_out_pk = 0, an_out_ita = 0, an_out_bd = 0, an_out_mom = 0;   // an analysis enqueued by olx_solution_analyze_begin
    // heterogeneous medium (kernel 2h)
    bool hetero = false; HeteroParams hp{}; DevBuf<float4> d_med; DevBuf<int> d_plane_k, d_plane_of_k;
    DevBuf<float> d_inv2z; DevBuf<int> d_kfirst, d_klast;
    int planes_per_layer = 1;                  // olx_field_medium_layering: 1 = one sample per plane (default)
    int plan_ppl = 1;                          // ... as seen by the last olx_field_set_medium: the layering its plan was built with
    DevBuf<float4> d_med_layer; DevBuf<int> d_layer_lo, d_layer_hi;
    // marched ray sums (kernel 2m): model requested for the next olx_field_set_medium, decision, double-buffered U[element][i][j]
    int medium_model = 0;                      // OLX_MEDIUM_AUTO / _SAMPLED / _MARCHED
    bool march_one = false;                    // kernel 2m: a' = kappa sig everywhere -> ONE running sum per ray (hp.kappa)
    DevBuf<float2> d_Utex;   // kernel 2m, one-sum form: the last running sums as row pairs {U(i,j), U(i+1,j)} (one 16-byte load per look-up above the medium)
    bool marched = false; DevBuf<float2> d_U[2]; std::vector<int> h_plane_k;
    DevBuf<float> d_sig;                      // kernel 2m, one-sum form: the planes' own terms as ONE float per cell, sig[plane][i][j] (the fused writers read them coalesced)
    int nbuf = 1; int cur = 0;
    std::string variant;
    std::vector<hipEvent_t> prof_ev; int prof_n = 0; bool prof_on = false;
    // pulsed model (kernel 2p): the setting of olx_field_pulse for the plans that follow, and what the current plan holds
    double pulse_cycles = 0, pulse_dt = 0; int pulse_nt = 0;   // n_t = 0: continuous wave
    double pulse_plan_dt = 0;                  // dt the current pulsed plan was built with (pulse holds everything else of it)
    bool pulsed = false;                       // the current plan is pulsed: d_pmag holds p_min
    bool pmax_live = false;                    // d_pmax holds the launched (and possibly scaled) p_max volumes
    bool agg_pmax_valid = false;               // d_agg_pmax holds max_f p_max_f of them
    PulseParams pulse{};
    DevBuf<float> d_pmax, d_agg_pmax;
    DevBuf<double4> d_ptab; DevBuf<float> d_pw;
    bool pii_live = false;                     // d_pii holds the pulse intensity integrals of the last launch (OLX_OUT_PII) or of olx_pii_upload, as scaled since by olx_pii_post
    int pii_foci = 0;                          // ... of this many foci
    long long pii_vox = 0;                     // voxels per volume the PII group below is sized for (pii_regrid frees it when the grid changes)
    DevBuf<float> d_pii;                       // [F * voxels], allocated only for a plan with OLX_OUT_PII / by olx_pii_upload
    bool pii_w_valid = false, pii_max_valid = false;   // d_pii_w / d_pii_max hold sum_f w_f PII_f / max_f PII_f of the volumes as they are now
    DevBuf<float> d_pii_w, d_pii_max;          // [voxels] each, created by the first olx_pii_post that forms them
    DevBuf<float> d_pii_gw;                    // [2 * PII_MAXF] olx_pii_post: the gains g_f = (float)(s_f^2), then the weights
    DevBuf<double> d_pii_A;                    // [PII_MAXF * 12] ... its focal frames
    DevBuf<unsigned> d_pii_peak;               // [4 * PII_MAXF + 1] ... its peaks (bit patterns)
    DevBuf<long long> d_ptrace_vox; DevBuf<float> d_ptrace;   // olx_field_pulse_trace: the voxel list and [F][n_points][n_t] samples
    // drive impulse responses of the pulsed model (olx_field_pulse_response, field_pulse_k<.., RESP>): the setting for the plans that follow
    // (host, fp64 taps as given) and what the current pulsed plan holds (presp_classes = 0: the plain kernel)
    std::vector<int> resp_cls, resp_row; std::vector<double> resp_taps;      // empty: no response
    int presp_classes = 0, presp_taps = 0, presp_hist = 0;                  // classes, taps in all, M_max - 1
    DevBuf<int> d_presp_tab;                   // [N] class of each element, then [classes + 1] first tap of each class
    DevBuf<float> d_presp_gam;                 // [taps][2] gamma_r[m] = g_r[m] e^{-j 2 pi frac(f0 dt m)} of the plan's f0 dt
    // pulsed model through a medium (kernel 2ph, olx_field_pulse_medium): buffers of their own, apart from the CW medium (`hetero`, d_med, d_inv2z ...)
    bool pulse_med = false;                    // the current pulsed plan launches kernel 2ph (until the next plan or upload)
    int pulse_med_R = 0;                       // its cache slots per lane: 4 (N <= 256) or 16 (N <= 1024)
    PulseMedParams pm{};
    DevBuf<double> d_pm_sig;                   // [n_planes][nx][ny] sigma = c_ref / c - 1 (fp64) of the non-trivial planes; not created without a sound-speed volume
    DevBuf<float> d_pm_att;                    // [n_planes][nx][ny] a [Np/m]; not created without an attenuation volume
    bool pm_has_sig = false, pm_has_att = false, pm_has_z = false;
    DevBuf<int> d_pm_plane_k, d_pm_plane_of_k; // [n_planes] grid plane of a held plane; [nz] held plane of a grid plane, -1 = trivial
    DevBuf<int2> d_pm_kb;                      // [N] { kfirst, klast } per element (the host's fp64 decisions)
    DevBuf<float> d_pm_inv2z;                  // [voxels] 1e-4 / (2 rho(v) c(v)); created with a sound-speed or density volume
    // thermal model (kernel 3, olx_thermal_*): buffers of their own, apart from the field / aggregate volumes
    bool th_planned = false, th_uniform = false; ThermalParams th{};
    double th_rate = 0;                        // max_v (sum_faces K + W) / (rho Cp)_v [1/s]: the FTCS bound is dt <= 1 / th_rate
    DevBuf<float> d_th_T[2]; int th_cur = 0; DevBuf<float> d_th_max, d_th_cem;
    DevBuf<float4> d_th_coef; DevBuf<float> d_th_irc, d_th_sfac; DevBuf<unsigned> d_th_rate;
    int th_steps = 0, th_max_focus = -1; std::vector<int> th_row; DevBuf<int> d_th_sf; DevBuf<float> d_th_tau;
    int th_npts = 0; DevBuf<long long> d_th_pts; DevBuf<float> d_th_trace;
    int th_src_foci = 0; bool th_src_resident = false; DevBuf<float> d_th_I;
    bool th_src_pii = false;                   // with th_src_resident: the resident PII volumes (olx_thermal_source_pii), not the intensity
    int th_next = -1;                          // the step the next olx_thermal_run continues with (-1: nothing run since the last plan / schedule)
    // full-wave model (kernel 5, olx_fullwave_*): buffers of their own, apart from the plan, the resident result and the thermal buffers
    bool fw_planned = false, fw_uniform = false; FullwaveParams fw{}; double fw_dt = 0, fw_dt_max = 0;
    DevBuf<float> d_fw_p, d_fw_v[3], d_fw_pmax, d_fw_pmin, d_fw_psq;   // [voxels] state p, v_x / v_y / v_z; p_max, p_min; sum p~^2 (created by the first run that asks for it)
    DevBuf<float> d_fw_coef[5];               // [voxels] b_x, b_y, b_z, kp, ga of a heterogeneous medium (not created for a uniform one)
    DevBuf<float> d_fw_dtab;                  // [nx + ny + nz] the layers' per-step decay d_x | d_y | d_z
    // split layers (olx_fullwave_layers; every olx_fullwave_plan returns to the sponge): the plan's layer arguments, the two tables per axis, and the
    // pressure components of the layer voxels, stored for the whole padded grid (an interior voxel's entries are never read or written)
    int fw_layers = 0, fw_pml = 0; double fw_pml_alpha = 0, fw_c_ref = 0;
    DevBuf<float> d_fw_rtab, d_fw_stab;       // [nx + ny + nz] r_x | r_y | r_z (centre depth), s_x | s_y | s_z (+ face depth); created by the first split model
    DevBuf<float> d_fw_pc[3];                 // [voxels] p_x, p_y, p_z; created by the first split model
    bool fw_sourced = false; FullwaveSource fw_src{}; int fw_entries = 0, fw_steps = 0;
    DevBuf<long long> d_fw_svox; DevBuf<int> d_fw_srow; DevBuf<double> d_fw_samp, d_fw_stau;   // CSR source table: voxel per row, row offsets, entries in table order
    // element-factored sources (olx_fullwave_sources_elements): the CSR table above holds amp_{e,m}, d_fw_sel the element of each entry, and the drive
    // s_e(n) of every (step, element) stands in a table that olx_fullwave_drive re-fills; fw_elem says which inject kernel olx_fullwave_run launches
    bool fw_elem = false; int fw_nel = 0;
    DevBuf<int> d_fw_sel; DevBuf<double> d_fw_drive, d_fw_dA, d_fw_dtau;   // [entries] element; [fw_steps][fw_nel] drive; [fw_nel] A_e, tau_e
    // what fills the drive table: 0 the bare burst, 1 the burst through the classes' drive taps (olx_fullwave_drive_response: fullwave_drive_k
    // fills the extended bare table, fullwave_drive_fir_k sums it), 2 a sampled table as uploaded (olx_fullwave_drive_table).  Every source call,
    // olx_fullwave_layers and olx_fullwave_plan return to 0.
    int fw_drive_mode = 0, fw_resp_classes = 0, fw_resp_ntaps = 0, fw_resp_mmax = 0;
    DevBuf<int> d_fw_gcls, d_fw_grow; DevBuf<double> d_fw_gtaps;   // [fw_nel] class of each element; [classes + 1] row offsets; [fw_resp_ntaps] taps
    DevBuf<double> d_fw_dext;                 // [fw_nel][fw_steps + fw_resp_mmax - 1] bare drive of the steps -(fw_resp_mmax - 1) .. fw_steps - 1, element-major
    // aperture weights (olx_fullwave_apertures): the planned grid in fp64, per-element geometry and index box, the dense weights of every box
    double fw_h[3] = {0, 0, 0}, fw_origin[3] = {0, 0, 0};
    DevBuf<FullwaveAperture> d_fw_ap; DevBuf<double> d_fw_apw;   // [elements]; [sum of the boxes' voxels]
    int fw_npts = 0; DevBuf<long long> d_fw_pts; DevBuf<float> d_fw_trace;   // trace voxels, [fw_steps][fw_npts] samples
    // lock-in at one frequency over the steps [fw_lock_w0, fw_lock_w0 + fw_lock_nw) (olx_fullwave_lockin; cleared by olx_fullwave_sources)
    bool fw_lock = false, fw_lock_vol = false; double fw_lock_freq = 0; int fw_lock_w0 = 0, fw_lock_nw = 0, fw_lock_nrec = 0, fw_lock_entries = 0;
    DevBuf<float> d_fw_lc, d_fw_ls;           // [voxels] sum p~ cos theta_n, sum p~ sin theta_n (created by the first lock-in that asks for the volume)
    DevBuf<int> d_fw_lrow; DevBuf<long long> d_fw_lvox; DevBuf<double> d_fw_lw, d_fw_lrc, d_fw_lrs;   // CSR receiver table: row offsets, voxels, weights; [receivers] sums
    int fw_next = -1; bool fw_pii = false;    // the step the next olx_fullwave_run continues with (-1: nothing run since the last plan / sources); the run accumulates sum p~^2
    // eikonal travel times (kernel 6, olx_eikonal_*): buffers of their own, apart from the plan, the resident result, the thermal and the full-wave buffers
    bool ek_solved = false; EikonalParams ek{}; int ek_cur = 0;   // a converged field stands in d_ek_T[ek_cur]
    DevBuf<float> d_ek_T[2];                  // [voxels] the ping-pong travel times [s], +inf = nothing arrived
    DevBuf<float> d_ek_c;                     // [voxels] the sound-speed volume of the running solve (not created for a uniform one)
    DevBuf<int> d_ek_flag;                    // [max_sweeps] sweep n + 1 lowered a voxel
    DevBuf<int> d_ek_row; DevBuf<long long> d_ek_vox; DevBuf<double> d_ek_w, d_ek_out;   // CSR sample table: row offsets, voxels, weights; [points] T
    // steering map (kernel 4, olx_steer_map): result volumes and element records of their own -- they never alias the field, aggregate or PII buffers
    DevBuf<float> d_sm_p; DevBuf<int> d_sm_n;          // [voxels] focal pressure [Pa], active elements; created by the first call, reused by later ones
    DevBuf<double> d_sm_tabd; DevBuf<float> d_sm_tabf; // [N * STEER_TD], [N * STEER_TF] element records (olx_params.h)
    DevBuf<double> d_sm_ap;                            // [N * 5] local x axes and sizes (directivity)
    bool sm_valid = false; SteerParams sm{}; int sm_kind = 0; bool sm_dir = false;   // the last olx_steer_map (olx_steer_time repeats it; olx_set_elements ends it)
    // steering map through a medium (kernel 4h, olx_steer_map_medium): kernel 4's element records plus buffers of its own, created by the first call and reused
    DevBuf<float> d_smm_p; DevBuf<int> d_smm_n;        // [voxels] focal pressure [Pa], active elements
    DevBuf<float4> d_smm_med;                          // [n_planes][nx][ny][2] pre-gathered { sig, a' } stencil of the non-trivial planes (kernel 2h's layout)
    DevBuf<int> d_smm_plane_k, d_smm_plane_of_k;       // [n_planes] grid plane of a stencil plane; [nz] stencil plane of a grid plane, -1 = trivial
    DevBuf<float> d_smm_tabm;                          // [N * STEER_TM] { kfirst, klast, S, 1 / S } per element
    bool sm_medium = false; SteerMedParams smm{}; int smm_comp = 0; bool smm_phase = false;   // the last map was olx_steer_map_medium's (sm_valid, sm_kind, sm_dir are shared)
    // StraightRay delays (kernel 1m, olx_bf_set_medium / olx_bf_solve_medium): the non-trivial sigma planes in buffers of their own, apart from
    // the field plan's medium and volumes
    bool bm_set = false; BfMedParams bm{};
    DevBuf<double> d_bm_sig;        // [n_planes][nx][ny] sigma = c_ref / c - 1 (fp64)
    DevBuf<double> d_bm_zp;         // [n_planes] z of the held planes [m]
    DevBuf<int> d_bm_pk;            // [nz] held plane of grid plane k, -1 = sigma == 0 there
    std::vector<int> h_bm_pk;       // host copy of d_bm_pk (the plane pairs of the one-walk launch are merged from it)
    // MediumCompensated apodization (kernel 1a, olx_bf_set_attenuation / olx_bf_solve_compensated): the non-zero attenuation planes, again in
    // buffers of their own (ba.c holds the frequency [Hz] the attenuation was converted at)
    bool ba_set = false; BfMedParams ba{};
    DevBuf<double> d_ba_att;        // [n_planes][nx][ny] a [Np/m] (fp64)
    DevBuf<double> d_ba_zp;         // [n_planes] z of the held planes [m]
    DevBuf<int> d_ba_pk;            // [nz] held plane of grid plane k, -1 = a == 0 there
    std::vector<int> h_ba_pk;
    DevBuf<double> d_ba_h;          // [F][N] arrival amplitudes h_e of the last launch (scratch)
    // ... and the walk of both at once: the planes held by either volume (rebuilt when either medium changes)
    bool bc_valid = false; int bc_planes = 0;
    DevBuf<double> d_bc_zp;         // [bc_planes] z [m]
    DevBuf<int2> d_bc_walk;         // [bc_planes] (sigma plane, attenuation plane), -1 = not held there
    // comm: RCCL communicator, or the direct peer-to-peer transport (exactly one of comm / p2p is set once initialised)
    P2PState* p2p = nullptr;
    bool comm_active() const { return comm != nullptr || p2p != nullptr; }
    RcclApi rccl; olx_nccl_comm comm = nullptr; int nranks = 1, rank = 0;
    hipStream_t comm_stream = nullptr; hipEvent_t ev_field[NBUF] = {nullptr, nullptr};
    hipEvent_t ev_gather[NBUF] = {nullptr, nullptr}; bool gather_pending[NBUF] = {false, false};
    DevBuf<float> d_gather;
    hipEvent_t ev_agg = nullptr, ev_red = nullptr; bool reduce_pending = false;
    int agg_local = -1, agg_total = 0;        // olx_field_aggregate_counts: genuine local foci / global focus count (padding excluded)
    std::string rccl_path;                     // file the RCCL symbols were bound from
    // parameters of the last olx_bf_solve (olx_bf_time repeats it)
    bool bf_valid = false; double bf_c = 0, bf_scale = 1, bf_p0 = 0, bf_p1 = 0; int bf_kind = 0;
};

// olx_p2p.hip
bool olx_p2p_requested();                                  // OLX_GATHER=p2p
bool olx_p2p_is_id(const void* id_bytes);
int olx_p2p_unique_id(olx_ctx* c, void* id_bytes);
int olx_p2p_init(olx_ctx* c, const void* id_bytes, int nranks, int rank);
int olx_p2p_destroy(olx_ctx* c);
int olx_p2p_attached(olx_ctx* c);                          // ranks that have attached to the control block
int olx_p2p_export(olx_ctx* c, void* blob_out);
int olx_p2p_import(olx_ctx* c, const void* blobs);
int olx_p2p_allgather(olx_ctx* c);
int olx_p2p_before_overwrite(olx_ctx* c, int b);
int olx_p2p_drain(olx_ctx* c);
int olx_p2p_aggregate(olx_ctx* c, bool scatter, bool with_i);
int olx_p2p_aggregate_before_overwrite(olx_ctx* c);

static inline int fail(olx_ctx* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    if (c) c->err = buf;
    return code;
}
#define HIPCHK(c, call)                                                                  \
    do {                                                                                 \
        hipError_t e_ = (call);                                                          \
        if (e_ != hipSuccess)                                                            \
            return fail((c), e_ == hipErrorOutOfMemory ? OLX_ENOMEM : OLX_EHIP, "%s: %s", #call, \
                        hipGetErrorString(e_));                                          \
    } while (0)

template <class T> int DevBuf<T>::reserve(olx_ctx* c, size_t n) {
    if (cap >= n && p) return OLX_OK;
    release();
    n = std::max(n, (size_t)1);
    HIPCHK(c, hipMalloc((void**)&p, sizeof(T) * n));
    cap = n;
    return OLX_OK;
}

// The aggregate volumes, created lazily at the output volumes' capacity (the group is freed together: reserve_outputs in olx.hip)
static inline int reserve_aggregate(olx_ctx* c, bool with_p, bool with_i) {
    const size_t n = c->d_pmag[0].capacity();
    int rc = with_p ? c->d_agg_p.reserve(c, n) : OLX_OK;
    if (!rc && with_i) rc = c->d_agg_i.reserve(c, n);
    return rc;
}

// A plan or an upload puts a grid of `vox` voxels there: no PII is resident any more, and the PII group (the volumes, the weighted and
// the max volume) is freed when it was sized for another grid
static inline void pii_regrid(olx_ctx* c, long long vox) {
    c->pii_live = false; c->pii_w_valid = false; c->pii_max_valid = false;
    if (c->pii_vox != vox) { c->d_pii.release(); c->d_pii_w.release(); c->d_pii_max.release(); }
    c->pii_vox = vox;
}

// call-scoped device scratch: freed on every return path
struct DevScratch {
    void* p = nullptr;
    ~DevScratch() { if (p) hipFree(p); }
    template <class T> T* at(size_t byte_off) const { return reinterpret_cast<T*>(static_cast<unsigned char*>(p) + byte_off); }
};

// Quadrature points of an aperture (olx_fullwave_apertures, fullwave_aperture_k): the offset (i + 1/2) / n - 1/2 of point i of n along an
// in-plane axis, and coordinate `axis` of the point with offsets (sa, sb) in voxel units, within 1e-9 of a whole number = that number.
// Every operation is rounded on its own (no fused multiply-add), so the host's refusals, the kernel and the fp64 oracle see the same bits.
__host__ __device__ inline double fw_aperture_s(int i, int n) {
#pragma clang fp contract(off)
    return ((double)i + 0.5) / (double)n - 0.5;
}
__host__ __device__ inline double fw_aperture_q(const FullwaveAperture& E, double sa, double sb, int axis, double origin, double h) {
#pragma clang fp contract(off)
    const double ta = (sa * E.w) * E.u[axis], tb = (sb * E.l) * E.v[axis];
    const double q = (((E.c[axis] + ta) + tb) - origin) / h;
    const double near = rint(q);
    return fabs(q - near) <= 1e-9 ? near : q;
}
