// C-ABI of the MI355X-native openlifu hot path (declared in include/olx.h).
// Host side: context, device buffers, launch logic, RCCL (dlopen) reassembly.  The kernel-2 families live in
// their own translation units (k_*.hip, launchers in olx_launch.h); the small kernels are compiled here.
#include "olx_ctx.h"

#include <dlfcn.h>
#include <unistd.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <limits>
#include <thread>

#include "k_small.hip.h"
#include "olx_launch.h"
#include "olx_medium.h"
#include "olx_plan.h"
#include "k_toep.hip.h"

OLX_BOUNDS_READER(small)     // debug library: the bounds words of this unit's kernels (pii_post_k)

// A device table kept with a host copy of what it holds (`held`): uploaded only when `v` differs from that copy.  The copy runs on the
// context's stream, behind whatever is queued there, and is waited for (`v` may live on the caller's frame).
template <class T> static int upload_if_changed(olx_ctx* c, DevBuf<T>& d, std::vector<T>& held, const std::vector<T>& v) {
    if (d.capacity() < v.size() || !d) held.clear();      // (reserve takes a new block: it holds nothing yet)
    { int rc = d.reserve(c, v.size()); if (rc) return rc; }
    if (held.size() == v.size() && (v.empty() || !memcmp(held.data(), v.data(), sizeof(T) * v.size()))) return OLX_OK;
    HIPCHK(c, hipMemcpyAsync(d, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    held = v;
    return OLX_OK;
}

// olxmed::check_grid's verdict in the words of every entry point that takes a grid
static int grid_fail(olx_ctx* c, const char* who, olxmed::GridFault f) {
    return fail(c, OLX_EINVAL, f == olxmed::GRID_SIZE ? "%s: grid sizes must be >= 1" : "%s: grid spacing must be finite and > 0, origin finite", who);
}

extern "C" {

int olx_abi_version(void) { return OLX_ABI_VERSION; }

int olx_device_count(int* count) {
    if (!count) return OLX_EINVAL;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; return OLX_EHIP; }
    *count = n;
    return OLX_OK;
}

int olx_ctx_create(int device, olx_ctx** out) {
    if (!out) return OLX_EINVAL;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return OLX_EHIP;
    olx_ctx* c = new (std::nothrow) olx_ctx();
    if (!c) return OLX_ENOMEM;
    c->device = device;
    if (hipSetDevice(device) != hipSuccess ||
        hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return OLX_EHIP;
    }
    if (hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || c->n_cu <= 0) c->n_cu = 256;
    *out = c;
    return OLX_OK;
}

int olx_comm_destroy(olx_ctx* c);
}
static void free_fetch_lanes(olx_ctx* c);
extern "C" {

int olx_ctx_destroy(olx_ctx* c) {
    if (!c) return OLX_EINVAL;
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
    olx_comm_destroy(c);
    free_fetch_lanes(c);
    if (c->h_an) hipHostFree(c->h_an);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;     // (the device buffers free themselves)
    return OLX_OK;
}

const char* olx_last_error(const olx_ctx* c) { return c ? c->err.c_str() : "null context"; }

#ifdef OLX_DEBUG_BOUNDS   // debug build (k_types.hip.h): the kernels' index checks report here
extern "C" { int olx_dbg_bounds_cosetp(unsigned*); int olx_dbg_bounds_coset(unsigned*); int olx_dbg_bounds_toep(unsigned*); int olx_dbg_bounds_hmarch(unsigned*); int olx_dbg_bounds_pulse(unsigned*); int olx_dbg_bounds_thermal(unsigned*); int olx_dbg_bounds_bfmed(unsigned*); int olx_dbg_bounds_small(unsigned*); int olx_dbg_bounds_steer(unsigned*); int olx_dbg_bounds_steermed(unsigned*); int olx_dbg_bounds_pulsemed(unsigned*); int olx_dbg_bounds_fullwave(unsigned*); int olx_dbg_bounds_eikonal(unsigned*); }
static int report_bounds(olx_ctx* c) {
    struct { const char* name; int (*read)(unsigned*); } units[] = {{"2g (k_coset2.hip)", olx_dbg_bounds_cosetp}, {"2e (k_coset.hip)", olx_dbg_bounds_coset},
                                                                     {"2f (k_toep.hip)", olx_dbg_bounds_toep}, {"2m (k_hmarch.hip)", olx_dbg_bounds_hmarch},
                                                                     {"2p (k_pulse.hip)", olx_dbg_bounds_pulse}, {"3 (k_thermal.hip)", olx_dbg_bounds_thermal},
                                                                     {"1m / 1a (k_bfmed.hip)", olx_dbg_bounds_bfmed}, {"pii_post_k (k_small.hip.h)", olx_dbg_bounds_small}, {"4 (k_steer.hip)", olx_dbg_bounds_steer},
                                                                     {"4h (k_steer_med.hip)", olx_dbg_bounds_steermed}, {"2ph (k_pulse_med.hip)", olx_dbg_bounds_pulsemed}, {"5 (k_fullwave.hip)", olx_dbg_bounds_fullwave},
                                                                     {"6 (k_eikonal.hip)", olx_dbg_bounds_eikonal}};
    int rc = OLX_OK;
    for (auto& u : units) {
        unsigned w[4] = {0, 0, 0, 0};
        if (u.read(w) != 0) return fail(c, OLX_EHIP, "debug build: cannot read the bounds words of kernel %s", u.name);
        if (w[1] && rc == OLX_OK)
            rc = fail(c, OLX_ESTATE, "debug build: kernel %s made %u accesses outside their extent (skipped; site mask 0x%x; first: index %u, extent %u)", u.name, w[1], w[0], w[2], w[3]);
    }
    return rc;
}
#endif

int olx_sync(olx_ctx* c) {
    if (!c) return OLX_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->comm_stream) HIPCHK(c, hipStreamSynchronize(c->comm_stream));
#ifdef OLX_DEBUG_BOUNDS
    { int rc_ = report_bounds(c); if (rc_) return rc_; }
#endif
    if (c->p2p) return olx_p2p_drain(c);     // peer-to-peer gathers run on the transport's worker thread
    return OLX_OK;
}


// The aggregate buffers are about to be rewritten: an exchange of the previous aggregate that still reads them -- RCCL on the side
// stream, or peers pulling slices out of them over IPC -- has to be over.
static int aggregate_buffers_free(olx_ctx* c) {
    if (c->reduce_pending) { HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_red, 0)); c->reduce_pending = false; }
    if (c->p2p) return olx_p2p_aggregate_before_overwrite(c);
    return OLX_OK;
}

// p2p transport: this rank's output blocks (both buffers) and aggregate buffers are IPC-mapped by its peers, which pull from them on
// their OWN worker threads.  olx_sync / olx_p2p_drain only wait for this rank's pulls; before an exported buffer is FREED (a larger
// plan, an upload, the end of the communicator) or rewritten IN PLACE (scale, the fused post-pass) every peer must have finished the
// pulls it still owes: pulled[r][me] of the generation that last sat in the buffer, agg_done[r] of the last aggregate exchange.
// `buf` = one output buffer, or -1 = both output buffers and the aggregate buffers.  A failed wait (peer timed out / aborted) clears
// the pending mark all the same -- the communicator is unusable after OLX_ECOMM (include/olx.h), the buffers are not.
static int exported_buffers_quiesce(olx_ctx* c, int buf) {
    if (!c->p2p) return OLX_OK;
    int rc = OLX_OK;
    for (int b = 0; b < olx_ctx::NBUF; ++b) {
        if ((buf >= 0 && b != buf) || !c->gather_pending[b]) continue;
        const int r = olx_p2p_before_overwrite(c, b);
        c->gather_pending[b] = false;
        if (r && !rc) rc = r;
    }
    if (buf < 0) { const int r = olx_p2p_aggregate_before_overwrite(c); if (r && !rc) rc = r; }
    return rc;
}

// The output volumes: d_pmag[0, nbuf) of `total` floats, d_inten / d_cplx when wanted, at the capacity of d_pmag[0] like the aggregate
// volumes (reserve_aggregate).  The group is freed together when it is too small or a second buffer is missing -- after the peers'
// pulls from it are over when `quiesce` (p2p: the blocks are IPC-exported).
static int reserve_outputs(olx_ctx* c, size_t total, int nbuf, bool want_inten, bool want_cplx, bool quiesce) {
    if (c->d_pmag[0].capacity() < total || (nbuf == 2 && !c->d_pmag[1])) {
        if (quiesce) { int rc = exported_buffers_quiesce(c, -1); if (rc) return rc; }
        for (DevBuf<float>* b : {&c->d_pmag[0], &c->d_pmag[1], &c->d_inten, &c->d_cplx, &c->d_agg_p, &c->d_agg_i}) b->release();
    }
    int rc = OLX_OK;
    for (int b = 0; b < nbuf && !rc; ++b) rc = c->d_pmag[b].reserve(c, total);
    const size_t cap = c->d_pmag[0].capacity();
    if (!rc && want_inten) rc = c->d_inten.reserve(c, cap);
    if (!rc && want_cplx) rc = c->d_cplx.reserve(c, 2 * cap);
    return rc;
}

// The intensity volumes as a kernel argument: null in a plan that derives its intensity (the scans then form olx_inten from the |p| they load)
static inline float* inten_arg(const olx_ctx* c) { return c->derive_i ? nullptr : (float*)c->d_inten; }

// out[i] = olx_inten(pmag[i], ik): what a deriving plan's intensity IS, for the readers that want it in memory
__global__ __launch_bounds__(256) void field_inten_fill_k(const float* __restrict__ pmag, long long n, float ik, float* __restrict__ out) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = olx_inten(pmag[i], ik);
}
static inline void inten_fill(olx_ctx* c, const float* pmag, size_t n, float* out) {
    hipLaunchKernelGGL(field_inten_fill_k, dim3((unsigned)std::min<size_t>((n + 255) / 256, 8192)), dim3(256), 0, c->stream, pmag, (long long)n, c->fp.inten_scale, out);
}

// The rare readers of whole intensity volumes (a masked peak or point samples of the intensity, the thermal source, the fetch of all foci): in a deriving
// plan d_inten is reserved on their first call and filled from the current |p| volumes; it stays valid until the next launch, scaling or plan.
// Nothing on Protocol.calc_solution's default path comes here.
static int materialize_intensity(olx_ctx* c) {
    if (!c->derive_i || c->inten_live) return OLX_OK;
    const size_t total = (size_t)c->fp.vox * c->plan_foci;
    { int rc = c->d_inten.reserve(c, std::max(total, c->d_pmag[0].capacity())); if (rc) return rc; }
    inten_fill(c, c->d_pmag[c->cur], total, c->d_inten);
    HIPCHK(c, hipGetLastError());
    c->inten_live = true;
    return OLX_OK;
}

// ---- element table ---------------------------------------------------------------------
int olx_set_elements(olx_ctx* c, const double* pos_m, const double* normal, const double* area_m2, int n) {
    if (!c) return OLX_EINVAL;
    if (!pos_m || !normal || !area_m2 || n <= 0) return fail(c, OLX_EINVAL, "olx_set_elements: null pointer or n <= 0");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (n != c->n_el) {
        for (DevBuf<double>* b : {&c->d_pos, &c->d_nrm, &c->d_area}) b->release();
        int rc = c->d_pos.reserve(c, 3 * (size_t)n);
        if (!rc) rc = c->d_nrm.reserve(c, 3 * (size_t)n);
        if (!rc) rc = c->d_area.reserve(c, n);
        if (rc) return rc;
    }
    // AoS [N][3] (the caller's natural layout) -> SoA [3][N] (coalesced on device)
    std::vector<double> soa(3 * (size_t)n), nso(3 * (size_t)n);
    for (int e = 0; e < n; ++e)
        for (int a = 0; a < 3; ++a) {
            soa[(size_t)a * n + e] = pos_m[3 * e + a];
            nso[(size_t)a * n + e] = normal[3 * e + a];
        }
    HIPCHK(c, hipMemcpy(c->d_pos, soa.data(), sizeof(double) * 3 * n, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_nrm, nso.data(), sizeof(double) * 3 * n, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_area, area_m2, sizeof(double) * n, hipMemcpyHostToDevice));
    c->h_pos.swap(soa);
    c->h_area.assign(area_m2, area_m2 + n);
    c->h_nrm.assign(normal, normal + 3 * (size_t)n);
    c->h_xaxis.clear(); c->h_size.clear();     // apertures belong to an element table
    c->resp_cls.clear(); c->resp_row.clear(); c->resp_taps.clear();      // ... and so do the drive impulse responses
    c->n_el = n;
    c->sm_valid = false;
    c->n_foci = 0;      // steering shape depends on N
    c->planned = false;
    c->steer_version++;
    return OLX_OK;
}

// ---- kernel 1 -----------------------------------------------------------------------------
int olx_set_element_apertures(olx_ctx* c, const double* xaxis, const double* size_m) {
    if (!c) return OLX_EINVAL;
    if (c->n_el <= 0) return fail(c, OLX_ESTATE, "olx_set_element_apertures: call olx_set_elements first");
    if (!xaxis || !size_m) return fail(c, OLX_EINVAL, "olx_set_element_apertures: null pointer");
    const int n = c->n_el;
    for (int e = 0; e < n; ++e) {
        const double* x = xaxis + 3 * e; const double* nr = c->h_nrm.data() + 3 * e;
        const double nx = std::sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]), dot = x[0] * nr[0] + x[1] * nr[1] + x[2] * nr[2];
        if (!(std::fabs(nx - 1.0) <= 1e-9) || !(std::fabs(dot) <= 1e-9))
            return fail(c, OLX_EINVAL, "olx_set_element_apertures: element %d: xaxis must be a unit vector orthogonal to the normal", e);
        if (!(size_m[2 * e] >= 0) || !(size_m[2 * e + 1] >= 0)) return fail(c, OLX_EINVAL, "olx_set_element_apertures: element %d: negative size", e);
    }
    c->h_xaxis.assign(xaxis, xaxis + 3 * (size_t)n);
    c->h_size.assign(size_m, size_m + 2 * (size_t)n);
    c->planned = false;
    return OLX_OK;
}

int olx_bf_solve(olx_ctx* c, const double* foci_m, int n_foci, const double* M, double cs, int apod_kind,
                 double p0, double p1, double* delays_out, double* apod_out) {
    if (!c) return OLX_EINVAL;
    if (c->n_el <= 0) return fail(c, OLX_ESTATE, "olx_bf_solve: call olx_set_elements first");
    if (!foci_m || n_foci <= 0) return fail(c, OLX_EINVAL, "olx_bf_solve: no foci");
    if (!(cs > 0)) return fail(c, OLX_EINVAL, "olx_bf_solve: speed of sound must be > 0");
    const double angle_scale = (apod_kind & OLX_APOD_RADIANS) ? 1.0 : (180.0 / 3.14159265358979323846);
    apod_kind &= ~OLX_APOD_RADIANS;
    if (apod_kind < 0 || apod_kind > 2) return fail(c, OLX_EINVAL, "olx_bf_solve: unknown apod_kind %d", apod_kind);
    if (apod_kind == OLX_APOD_PIECEWISE && !(p1 < p0)) return fail(c, OLX_EINVAL, "olx_bf_solve: rolloff must be < zero angle");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t fn = (size_t)n_foci * c->n_el;
    int rc = c->d_delays.reserve(c, fn);
    if (!rc) rc = c->d_apod.reserve(c, fn);
    if (!rc) rc = c->d_foci.reserve(c, 3 * (size_t)n_foci);
    if (!rc) rc = c->d_M.reserve(c, 16);
    if (rc) return rc;
    static const double I4[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    HIPCHK(c, hipMemcpyAsync(c->d_foci, foci_m, sizeof(double) * 3 * n_foci, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_M, M ? M : I4, sizeof(double) * 16, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(bf_solve_k, dim3(n_foci), dim3(BF_THREADS), 0, c->stream, c->d_pos, c->d_nrm, c->n_el,
                       c->d_foci, c->d_M, cs, apod_kind, angle_scale, p0, p1, c->d_delays, c->d_apod);
    HIPCHK(c, hipGetLastError());
    c->h_delays.resize(fn); c->h_apod.resize(fn);
    HIPCHK(c, hipMemcpyAsync(c->h_delays.data(), c->d_delays, sizeof(double) * fn, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->h_apod.data(), c->d_apod, sizeof(double) * fn, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (delays_out) memcpy(delays_out, c->h_delays.data(), sizeof(double) * fn);
    if (apod_out) memcpy(apod_out, c->h_apod.data(), sizeof(double) * fn);
    c->n_foci = n_foci;
    c->steer_version++;
    c->bf_c = cs; c->bf_kind = apod_kind; c->bf_scale = angle_scale; c->bf_p0 = p0; c->bf_p1 = p1; c->bf_valid = true;
    c->h_foci.clear();
    if (!M || !memcmp(M, I4, sizeof I4)) {   // focus positions are in the frame of the element table: usable for planning decisions
        c->h_foci.assign(foci_m, foci_m + 3 * (size_t)n_foci);
        c->foci_version = c->steer_version;
    }
    return OLX_OK;
}

int olx_bf_time(olx_ctx* c, int iters, float* us_each) {
    if (!c) return OLX_EINVAL;
    if (iters < 1 || !us_each) return fail(c, OLX_EINVAL, "olx_bf_time: iters < 1 or null output");
    if (!c->bf_valid || c->n_foci <= 0) return fail(c, OLX_ESTATE, "olx_bf_time: no olx_bf_solve to repeat");
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<hipEvent_t> ev(iters + 1, nullptr);
    for (auto& e : ev) HIPCHK(c, hipEventCreate(&e));
    HIPCHK(c, hipEventRecord(ev[0], c->stream));
    for (int i = 0; i < iters; ++i) {   // same foci, transform and options as the last solve: the outputs are rewritten with equal values
        hipLaunchKernelGGL(bf_solve_k, dim3(c->n_foci), dim3(BF_THREADS), 0, c->stream, c->d_pos, c->d_nrm, c->n_el,
                           c->d_foci, c->d_M, c->bf_c, c->bf_kind, c->bf_scale, c->bf_p0, c->bf_p1, c->d_delays, c->d_apod);
        HIPCHK(c, hipEventRecord(ev[i + 1], c->stream));
    }
    hipError_t e = hipStreamSynchronize(c->stream);
    for (int i = 0; i < iters && e == hipSuccess; ++i) { float ms = 0; e = hipEventElapsedTime(&ms, ev[i], ev[i + 1]); us_each[i] = ms * 1e3f; }
    for (auto& v : ev) hipEventDestroy(v);
    if (e != hipSuccess) return fail(c, OLX_EHIP, "olx_bf_time: %s", hipGetErrorString(e));
    return OLX_OK;
}

// ---- kernel 1m: StraightRay delays through a medium ------------------------------------------------------------------
// the grid part of kernel 1m's / 1a's parameters; `value` = the reference sound speed (1m) or the frequency (1a)
static void bfmed_params(BfMedParams& P, const olx_grid& g, double value, int n_planes) {
    P.ox = g.origin[0]; P.oy = g.origin[1]; P.oz = g.origin[2];
    P.hx = g.spacing[0]; P.hy = g.spacing[1]; P.hz = g.spacing[2];
    P.dmin = 0.5 * std::min(P.hx, std::min(P.hy, P.hz));
    P.ztol = 1e-6 * P.hz;
    P.c = value;
    P.nx = g.n[0]; P.ny = g.n[1]; P.nz = g.n[2]; P.n_planes = n_planes;
}
int olx_bf_set_medium(olx_ctx* c, const float* sound_speed, const olx_grid* grid, double c_ref) {
    if (!c) return OLX_EINVAL;
    if (!grid) return fail(c, OLX_EINVAL, "olx_bf_set_medium: null grid");
    if (!(c_ref > 0) || !std::isfinite(c_ref)) return fail(c, OLX_EINVAL, "olx_bf_set_medium: c_ref must be finite and > 0");
    if (auto f = olxmed::check_grid(*grid)) return grid_fail(c, "olx_bf_set_medium", f);
    const int nx = grid->n[0], ny = grid->n[1], nz = grid->n[2];
    const size_t nxy = (size_t)nx * ny;
    if (olxmed::first_bad(sound_speed, nxy * nz, olxmed::POSITIVE) < nxy * nz) return fail(c, OLX_EINVAL, "olx_bf_set_medium: sound speed must be finite and > 0");
    // the held planes: olxmed::scan_planes_columns, scan_planes' rule for the sound speed (a plane with any voxel != c_ref), sigma = c_ref / c - 1 in fp64
    std::vector<double> zp, sig;
    olxmed::Planes pl = olxmed::scan_planes_columns(sound_speed, c_ref, nullptr, 0.0, nx, ny, nz, sig);
    for (int k : pl.plane_k) zp.push_back(grid->origin[2] + k * grid->spacing[2]);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));      // (a solve of the previous medium may still read the buffers)
    c->bm_set = false; c->bc_valid = false;
    int rc = c->d_bm_sig.reserve(c, sig.size());
    if (!rc) rc = c->d_bm_zp.reserve(c, zp.size());
    if (!rc) rc = c->d_bm_pk.reserve(c, nz);
    if (rc) return rc;
    if (!sig.empty()) HIPCHK(c, hipMemcpy(c->d_bm_sig, sig.data(), sizeof(double) * sig.size(), hipMemcpyHostToDevice));
    if (!zp.empty()) HIPCHK(c, hipMemcpy(c->d_bm_zp, zp.data(), sizeof(double) * zp.size(), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_bm_pk, pl.plane_of_k.data(), sizeof(int) * nz, hipMemcpyHostToDevice));
    bfmed_params(c->bm, *grid, c_ref, (int)zp.size());
    c->h_bm_pk.swap(pl.plane_of_k);
    c->bm_set = true;
    return OLX_OK;
}

int olx_bf_solve_medium(olx_ctx* c, const double* foci_m, int n_foci, const double* M, double cs, int apod_kind,
                        double p0, double p1, double* delays_out, double* apod_out) {
    if (!c) return OLX_EINVAL;
    if (!c->bm_set) return fail(c, OLX_ESTATE, "olx_bf_solve_medium: call olx_bf_set_medium first");
    if (c->n_el <= 0) return fail(c, OLX_ESTATE, "olx_bf_solve_medium: call olx_set_elements first");
    if (!foci_m || n_foci <= 0) return fail(c, OLX_EINVAL, "olx_bf_solve_medium: no foci");
    if (cs != c->bm.c) return fail(c, OLX_EINVAL, "olx_bf_solve_medium: c (%.17g) must be the c_ref of olx_bf_set_medium (%.17g)", cs, c->bm.c);
    for (size_t q = 0; q < 3 * (size_t)n_foci; ++q)
        if (!std::isfinite(foci_m[q])) return fail(c, OLX_EINVAL, "olx_bf_solve_medium: focus positions must be finite");
    for (int q = 0; M && q < 16; ++q)
        if (!std::isfinite(M[q])) return fail(c, OLX_EINVAL, "olx_bf_solve_medium: transform must be finite");
    // kernel 1 (the apodization, the foci and the transform on the device), then kernel 1m over its delays
    int rc = olx_bf_solve(c, foci_m, n_foci, M, cs, apod_kind, p0, p1, nullptr, apod_out);
    if (rc) return rc;
    olx_launch_bfmed(c, n_foci);
    HIPCHK(c, hipGetLastError());
    const size_t fn = (size_t)n_foci * c->n_el;
    HIPCHK(c, hipMemcpyAsync(c->h_delays.data(), c->d_delays, sizeof(double) * fn, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (delays_out) memcpy(delays_out, c->h_delays.data(), sizeof(double) * fn);
    c->steer_version++;
    c->h_foci.clear();      // not geometric delays: the planner must not take the foci as known (infer_foci decides)
    c->bf_valid = false;    // (olx_bf_time would rewrite the table with kernel 1's delays)
    return OLX_OK;
}

// ---- kernel 1a: MediumCompensated apodization through a medium ---------------------------------------------------------
int olx_bf_set_attenuation(olx_ctx* c, const float* att, const olx_grid* grid, double freq_hz) {
    if (!c) return OLX_EINVAL;
    if (!grid) return fail(c, OLX_EINVAL, "olx_bf_set_attenuation: null grid");
    if (!(freq_hz > 0) || !std::isfinite(freq_hz)) return fail(c, OLX_EINVAL, "olx_bf_set_attenuation: freq_hz must be finite and > 0");
    if (auto f = olxmed::check_grid(*grid)) return grid_fail(c, "olx_bf_set_attenuation", f);
    const int nx = grid->n[0], ny = grid->n[1], nz = grid->n[2];
    const size_t nxy = (size_t)nx * ny;
    if (olxmed::first_bad(att, nxy * nz, olxmed::NON_NEGATIVE) < nxy * nz) return fail(c, OLX_EINVAL, "olx_bf_set_attenuation: attenuation must be finite and >= 0");
    // the held planes: olxmed::scan_planes_columns, scan_planes' rule for the attenuation (a plane with any voxel != 0), a [Np/m] in fp64 (sim/field.py _np_per_m)
    std::vector<double> zp, av;
    olxmed::Planes pl = olxmed::scan_planes_columns(nullptr, 0.0, att, std::pow(freq_hz * 1e-6, 0.9), nx, ny, nz, av);
    for (int k : pl.plane_k) zp.push_back(grid->origin[2] + k * grid->spacing[2]);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));      // (a solve of the previous attenuation may still read the buffers)
    c->ba_set = false; c->bc_valid = false;
    int rc = c->d_ba_att.reserve(c, av.size());
    if (!rc) rc = c->d_ba_zp.reserve(c, zp.size());
    if (!rc) rc = c->d_ba_pk.reserve(c, nz);
    if (rc) return rc;
    if (!av.empty()) HIPCHK(c, hipMemcpy(c->d_ba_att, av.data(), sizeof(double) * av.size(), hipMemcpyHostToDevice));
    if (!zp.empty()) HIPCHK(c, hipMemcpy(c->d_ba_zp, zp.data(), sizeof(double) * zp.size(), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_ba_pk, pl.plane_of_k.data(), sizeof(int) * nz, hipMemcpyHostToDevice));
    bfmed_params(c->ba, *grid, freq_hz, (int)zp.size());
    c->h_ba_pk.swap(pl.plane_of_k);
    c->ba_set = true;
    return OLX_OK;
}

// the planes held by either medium, in z order, with their plane in each: what the one-walk launch of kernels 1m + 1a steps through
static int build_joint_walk(olx_ctx* c) {
    const int nz = c->bm.nz;
    std::vector<double> zp;
    std::vector<int2> walk;
    for (int k = 0; k < nz; ++k) {
        const int ps = c->h_bm_pk[k], pa = c->h_ba_pk[k];
        if (ps < 0 && pa < 0) continue;
        zp.push_back(c->bm.oz + k * c->bm.hz);      // (olx_bf_set_medium's expression for its planes)
        walk.push_back(make_int2(ps, pa));
    }
    int rc = c->d_bc_zp.reserve(c, zp.size());
    if (!rc) rc = c->d_bc_walk.reserve(c, walk.size());
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (!zp.empty()) {
        HIPCHK(c, hipMemcpy(c->d_bc_zp, zp.data(), sizeof(double) * zp.size(), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(c->d_bc_walk, walk.data(), sizeof(int2) * walk.size(), hipMemcpyHostToDevice));
    }
    c->bc_planes = (int)zp.size();
    c->bc_valid = true;
    return OLX_OK;
}

int olx_bf_solve_compensated(olx_ctx* c, const double* foci_m, int n_foci, const double* M, double cs, int apod_kind,
                             double p0, double p1, int mode, int spreading, int use_delay_medium, double* delays_out, double* apod_out) {
    if (!c) return OLX_EINVAL;
    if (!c->ba_set) return fail(c, OLX_ESTATE, "olx_bf_solve_compensated: call olx_bf_set_attenuation first");
    if (use_delay_medium && !c->bm_set) return fail(c, OLX_ESTATE, "olx_bf_solve_compensated: call olx_bf_set_medium first (use_delay_medium)");
    if (c->n_el <= 0) return fail(c, OLX_ESTATE, "olx_bf_solve_compensated: call olx_set_elements first");
    if (!foci_m || n_foci <= 0) return fail(c, OLX_EINVAL, "olx_bf_solve_compensated: no foci");
    if (mode != OLX_COMP_EQUALIZE && mode != OLX_COMP_MATCHED) return fail(c, OLX_EINVAL, "olx_bf_solve_compensated: unknown mode %d", mode);
    if (use_delay_medium) {
        const BfMedParams &a = c->bm, &b = c->ba;
        if (cs != a.c) return fail(c, OLX_EINVAL, "olx_bf_solve_compensated: c (%.17g) must be the c_ref of olx_bf_set_medium (%.17g)", cs, a.c);
        if (a.nx != b.nx || a.ny != b.ny || a.nz != b.nz || a.ox != b.ox || a.oy != b.oy || a.oz != b.oz || a.hx != b.hx || a.hy != b.hy || a.hz != b.hz)
            return fail(c, OLX_EINVAL, "olx_bf_solve_compensated: the media of olx_bf_set_medium and olx_bf_set_attenuation must share one grid");
    }
    for (size_t q = 0; q < 3 * (size_t)n_foci; ++q)
        if (!std::isfinite(foci_m[q])) return fail(c, OLX_EINVAL, "olx_bf_solve_compensated: focus positions must be finite");
    for (int q = 0; M && q < 16; ++q)
        if (!std::isfinite(M[q])) return fail(c, OLX_EINVAL, "olx_bf_solve_compensated: transform must be finite");
    // kernel 1 (delays, the base apodization, the foci and the transform on the device), then ONE walk of the rays over its table
    int rc = olx_bf_solve(c, foci_m, n_foci, M, cs, apod_kind, p0, p1, nullptr, nullptr);
    if (rc) return rc;
    const size_t fn = (size_t)n_foci * c->n_el;
    rc = c->d_ba_h.reserve(c, fn);
    if (!rc && use_delay_medium && !c->bc_valid) rc = build_joint_walk(c);
    if (rc) { c->n_foci = 0; return rc; }
    olx_launch_bfapod(c, n_foci, mode, spreading != 0, use_delay_medium != 0);
    HIPCHK(c, hipGetLastError());
    if (use_delay_medium) HIPCHK(c, hipMemcpyAsync(c->h_delays.data(), c->d_delays, sizeof(double) * fn, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->h_apod.data(), c->d_apod, sizeof(double) * fn, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (delays_out) memcpy(delays_out, c->h_delays.data(), sizeof(double) * fn);
    if (apod_out) memcpy(apod_out, c->h_apod.data(), sizeof(double) * fn);
    c->steer_version++;
    if (use_delay_medium) c->h_foci.clear();      // not geometric delays (as olx_bf_solve_medium)
    else if (!c->h_foci.empty()) c->foci_version = c->steer_version;      // kernel 1's delays: the foci stay known, the planner reads the apodization as data
    c->bf_valid = false;    // (olx_bf_time would rewrite the table with kernel 1's apodization)
    return OLX_OK;
}

int olx_set_steering(olx_ctx* c, const double* delays_s, const double* apod, int n_foci) {
    if (!c) return OLX_EINVAL;
    if (c->n_el <= 0) return fail(c, OLX_ESTATE, "olx_set_steering: call olx_set_elements first");
    if (!delays_s || !apod || n_foci <= 0) return fail(c, OLX_EINVAL, "olx_set_steering: null pointer or n_foci <= 0");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t fn = (size_t)n_foci * c->n_el;
    int rc = c->d_delays.reserve(c, fn);
    if (!rc) rc = c->d_apod.reserve(c, fn);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->d_delays, delays_s, sizeof(double) * fn, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_apod, apod, sizeof(double) * fn, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->h_delays.assign(delays_s, delays_s + fn); c->h_apod.assign(apod, apod + fn);
    c->h_foci.clear();   // external delays: where the foci are is not known
    c->bf_valid = false;
    c->n_foci = n_foci;
    c->steer_version++;
    return OLX_OK;
}

int olx_bf_quantize(olx_ctx* c, double bf_clk_hz, int width_bits, uint16_t* ticks_out, uint8_t* apod_off_out,
                    double* max_apod_out, int32_t* n_overflow_out) {
    if (!c) return OLX_EINVAL;
    if (c->n_foci <= 0) return fail(c, OLX_ESTATE, "olx_bf_quantize: no steering table (olx_bf_solve / olx_set_steering)");
    if (!(bf_clk_hz > 0) || width_bits < 1 || width_bits > 16) return fail(c, OLX_EINVAL, "olx_bf_quantize: bad clock or width");
    HIPCHK(c, hipSetDevice(c->device));
    const int F = c->n_foci, n = c->n_el;
    const size_t fn = (size_t)F * n;
    // one scratch allocation: [F] max apod (fp64) | [F] overflow counts | [F N] ticks | [F N] apod-off bytes
    DevScratch scratch;
    const size_t off_o = sizeof(double) * F, off_t = off_o + sizeof(int) * (size_t)((F + 1) & ~1), off_a = off_t + sizeof(unsigned short) * fn;
    HIPCHK(c, hipMalloc(&scratch.p, off_a + fn));
    double* d_m = scratch.at<double>(0);
    int* d_o = scratch.at<int>(off_o);
    unsigned short* d_t = scratch.at<unsigned short>(off_t);
    unsigned char* d_a = scratch.at<unsigned char>(off_a);
    hipLaunchKernelGGL(bf_quantize_k, dim3(F), dim3(BF_THREADS), 0, c->stream, c->d_delays, c->d_apod, n, bf_clk_hz,
                       (1u << width_bits) - 1u, d_t, d_a, d_m, d_o);
    int rc = OLX_OK;
    if (hipGetLastError() != hipSuccess) rc = fail(c, OLX_EHIP, "olx_bf_quantize: launch failed");
    if (!rc && ticks_out && hipMemcpyAsync(ticks_out, d_t, sizeof(unsigned short) * fn, hipMemcpyDeviceToHost, c->stream) != hipSuccess) rc = OLX_EHIP;
    if (!rc && apod_off_out && hipMemcpyAsync(apod_off_out, d_a, fn, hipMemcpyDeviceToHost, c->stream) != hipSuccess) rc = OLX_EHIP;
    if (!rc && max_apod_out && hipMemcpyAsync(max_apod_out, d_m, sizeof(double) * F, hipMemcpyDeviceToHost, c->stream) != hipSuccess) rc = OLX_EHIP;
    if (!rc && n_overflow_out && hipMemcpyAsync(n_overflow_out, d_o, sizeof(int) * F, hipMemcpyDeviceToHost, c->stream) != hipSuccess) rc = OLX_EHIP;
    if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) rc = OLX_EHIP;
    if (rc == OLX_EHIP) return fail(c, OLX_EHIP, "olx_bf_quantize: HIP error");
    return rc;
}

// ---- kernel 2 -----------------------------------------------------------------------------
// The pure planning code (lattice detection, K-slot map, mirror permutations, column packing, block records, store jobs, focus inference, the
// e4m3 rule, kernel 2f's block shape, and the variant decision that combines them) lives in olx_plan.cpp: no HIP in it, so the CPU suite runs
// it under AddressSanitizer / UBSan (tools/plan_check.cpp, tests/test_plan_host.py).
static void detect_lattice(olx_ctx* c, const double lo[3], const double hi[3], double dmin) {
    olxplan::detect_lattice(c->lat, c->flat, c->n_el, c->h_pos.data(), c->grid.spacing, lo, hi, dmin);
}
static bool infer_foci(const olx_ctx* c, std::vector<double>& foci) {
    const int n = c->n_el, F = c->plan_foci;
    if (c->h_delays.size() != (size_t)F * n) return false;
    return olxplan::infer_foci(c->flat, n, F, c->h_pos.data(), c->h_delays.data(), c->c,
                               c->grid.origin[2] + 0.5 * (c->grid.n[2] - 1) * c->grid.spacing[2], foci);
}

static_assert(olxplan::FLAG_OUT_PMAG == OLX_OUT_PMAG && olxplan::FLAG_OUT_INTENSITY == OLX_OUT_INTENSITY && olxplan::FLAG_OUT_COMPLEX == OLX_OUT_COMPLEX &&
              olxplan::FLAG_FP16_CORRECTION == OLX_FIELD_FP16_CORRECTION, "olx_plan.h restates the plan flags");

// The pins of the variant decision, read from the environment once per decision.  OLX_FIELD_VARIANT pins a kernel family / form for A/B runs and
// OLX_FP8_CORRECTION=0 opts out of the e4m3 products like the plan flag.  Any other value of OLX_FP8_CORRECTION FORCES them past the eligibility
// rule -- results may then miss the 1e-5 gate, so only developer builds (OLX_DEV_PINS: the debug library, A/B timing builds) honour it, like
// the OLX_EXP_* switches; the product ignores them.
static olxplan::Pins read_pins() {
    olxplan::Pins pins;
    if (const char* fv = getenv("OLX_FIELD_VARIANT"))
        pins.family = !strcmp(fv, "lattice") ? olxplan::FamilyPin::lattice : !strcmp(fv, "lattice2d") ? olxplan::FamilyPin::lattice2d : olxplan::FamilyPin::other;
    const char* f8env = getenv("OLX_FP8_CORRECTION");
    if (f8env && !strcmp(f8env, "0")) pins.fp8 = -1;
#ifdef OLX_DEV_PINS
    if (f8env && strcmp(f8env, "0") != 0) pins.fp8 = 1;
    if (const char* e = getenv("OLX_EXP_TOEP_SAW")) { const int v = atoi(e); if (v >= 8 && v <= 24) pins.toep_saw = v; }   // (A/B)
    if (const char* e = getenv("OLX_EXP_TOEP_NM")) pins.toep_nm = atoi(e) == 3 ? 3 : 1;      // (A/B: 1 or 3)
    if (const char* e = getenv("OLX_EXP_KGRP")) pins.kgrp = std::max(1, atoi(e));
    { const char* e = getenv("OLX_EXP_CP_NOREUSE"); pins.cp_noreuse = e && atoi(e) != 0; }
    { const char* e = getenv("OLX_EXP_CP_NOFILLAHEAD"); pins.cp_nofillahead = e && atoi(e) != 0; }
    { const char* e = getenv("OLX_EXP_CP_NOSORT"); pins.cp_nosort = e && atoi(e) != 0; }
#endif
    return pins;
}

// Steering-dependent part of the kernel-2 variant choice (runs whenever the steering table changed), in two steps.  DECIDE: olxplan::decide_variant
// (olx_plan.cpp: pure host code) chooses the kernel family and its shape from what olx_field_plan established, the steering table and the pins, and
// fills the parameter blocks and tables.  APPLY: this function copies the plan into the context fields the launchers read, sizes the device buffers
// and uploads the tables.  No choice of a family or a shape is made here.
// (the result is remembered per steering version: olx_field_plan names the variant with it, the launch that follows packs against the same
// decisions instead of deriving them again -- column packing, block records and their uploads were 0.28 ms of every calc_solution, twice)
static int configure_variant(olx_ctx* c) {
    c->configured_version = ~0ull;
    const int n = c->n_el, F = c->plan_foci;
    const bool steering = c->h_delays.size() == (size_t)F * n && c->h_apod.size() == (size_t)F * n;
    olxplan::VariantIn in;
    in.n = n; in.F = F; in.pos = c->h_pos.data(); in.area = c->h_area.data();
    in.delays = steering ? c->h_delays.data() : nullptr; in.apod = steering ? c->h_apod.data() : nullptr;
    in.px = c->h_px.data(); in.py = c->h_py.data();
    in.freq = c->freq; in.c = c->c; in.p0_pa = c->p0_pa;
    for (int a = 0; a < 3; ++a) { in.origin[a] = c->grid.origin[a]; in.spacing[a] = c->grid.spacing[a]; in.gn[a] = c->grid.n[a]; }
    in.x_begin = c->slab.x_begin; in.x_count = c->slab.x_count; in.flags = c->flags; in.fp = c->fp;
    in.flat = c->flat; in.clamp = c->clamp; in.near = c->near; in.min_dist = c->min_dist; in.mx = c->mx; in.my = c->my;
    in.allow_shared = c->allow_shared; in.dir_lattice = c->dir_lattice; in.directivity = c->directivity; in.absorb_np_m = c->plan_absorb;      // (the plan's absorption, not a later olx_field_absorption)
    in.force_kind = c->force_kind;
    if (c->h_size.size() >= 2) { in.size0 = c->h_size[0]; in.size1 = c->h_size[1]; }
    in.hetero = c->hetero; in.marched = c->marched; in.march_one = c->march_one;
    in.n_planes = c->hp.n_planes; in.n_layers = c->hp.n_layers; in.planes_per_layer = c->plan_ppl;
    in.lat = &c->lat;
    in.pins = read_pins();
    if (olxplan::variant_reads_foci(in)) {      // the e4m3 rule wants the foci: known from olx_bf_solve in the element frame, or external delays that are geometric
        bool known = c->h_foci.size() == 3 * (size_t)F && c->foci_version == c->steer_version;
        if (!known && infer_foci(c, c->h_foci)) {
            c->foci_version = c->steer_version;
            known = true;
        }
        if (known) in.foci = c->h_foci.data();
    }
    int slot_rows = c->lat.nsbp;
    const olxplan::VariantPlan p = olxplan::decide_variant(in, c->nf_s2, slot_rows);
    if (slot_rows != c->lat.nsbp) olxplan::build_slot_map(c->lat, slot_rows);

    c->mx = p.mx; c->my = p.my; c->dx = p.dx; c->dy = p.dy; c->nf = p.nf; c->nt = p.nt;
    c->allow_shared = p.allow_shared; c->dir_lattice = p.dir_lattice;
    c->use_mfma = p.use_mfma; c->use_lattice = p.use_lattice; c->use_coset = p.use_coset; c->use_toep = p.use_toep; c->use_cosetp = p.use_cosetp;
    c->fp8corr = p.fp8corr;
    if (c->hetero) {
        { int rc = c->d_tab.reserve(c, (size_t)((F + c->nf - 1) / c->nf) * n * (HET_TAB_HEAD + 2 * c->nf)); if (rc) return rc; }
        c->hp.n_foci = F;
    } else if (p.use_mfma) {
        // (uploaded tables are remembered: an interactive caller re-plans per target, and a new target of the same focal pattern leaves the mirror
        // permutations, the columns' representatives and their store targets as they were -- no copies, no wait for the stream)
        { int rc = upload_if_changed(c, c->d_perm, c->up_perm, p.perm); if (rc) return rc; }
        { int rc = upload_if_changed(c, c->d_colinfo, c->up_colinfo, p.colinfo); if (rc) return rc; }
        c->d_targets = c->d_colinfo + p.colinfo.size() / 3;      // one table: the store targets are its second part
        c->fp8_kcut = p.fp8_kcut;
        c->bfrag_half = (size_t)p.mp.n_tiles * (p.n_pad / 16) * 128 * c->nt;      // uint4 per K-step and column tile: hi, lo of the 64 lanes
        {   // (index, residual) per element: kernel 2c; a second operand set in the other arithmetic for a launch split at fp8_kcut
            int rc = c->d_coords.reserve(c, 2 * (size_t)p.n_pad);
            if (!rc) rc = c->d_bfrag.reserve(c, 2 * c->bfrag_half);
            if (rc) return rc;
        }
        if (p.use_lattice) {     // (a new steering table alone changes no slot map)
            int rc = upload_if_changed(c, c->d_slot, c->up_slot, c->lat.slot_elem);
            if (rc) return rc;
            c->lat_mt = p.lat_mt; c->lp = p.lp;
        }
        c->mp = p.mp; c->mfma_wscale = p.mfma_wscale;
        if (p.use_lattice && p.use_coset) {
            c->cp = p.cp; c->toep_nm = p.toep.nm;
            if (p.use_cosetp) {
                // kernel 2g requests its steering fragments a table pair (two super-blocks) at a time under ONE block-uniform test and without per-lane
                // bounds: the super-block count of a launch tile is even, and each operand set (the second one, bfrag_half on, included) holds
                // n_tiles x nsa x nsbp whole super-blocks of 4 K-step records x 2 column tiles x 128 uint4
                const size_t n_sb = (size_t)p.cp.nsa * p.cp.nsbp;
                if (p.cp.nsa < 1 || p.cp.nsbp < 2 || p.cp.nsbp % 2 != 0)
                    return fail(c, OLX_ESTATE, "kernel 2g: %d x %d super-blocks: the steering requests need an even row count", p.cp.nsa, p.cp.nsbp);
                if (c->nt != 2 || c->bfrag_half != (size_t)p.mp.n_tiles * n_sb * 4 * 2 * 128)
                    return fail(c, OLX_ESTATE, "kernel 2g: the steering operands hold %zu uint4 per set, %d launch tiles x %zu super-blocks need %zu",
                                c->bfrag_half, p.mp.n_tiles, n_sb, (size_t)p.mp.n_tiles * n_sb * 4 * 2 * 128);
            }
            { int rc = upload_if_changed(c, c->d_jobs, c->up_jobs, p.jobs); if (rc) return rc; }
            {   // block records: they depend on the partition only, not on the steering table -- a call that changes nothing but the foci finds the
                // records it uploaded last time still valid
                std::vector<CosetBlock> blk;
                if (!c->up_blocks.empty() && memcmp(c->up_blocks_key, p.rec_key, sizeof p.rec_key) == 0) blk = c->up_blocks;
                else {
                    std::string why;
                    if (!olxplan::build_variant_blocks(p, blk, why)) return fail(c, OLX_ESTATE, "kernel 2g: %s", why.c_str());
                }
                const unsigned nblk = (unsigned)blk.size();
                c->cp_nfar = nblk - p.blocks_near;
                { int rc = upload_if_changed(c, c->d_cpblocks, c->up_blocks, blk); if (rc) return rc; }
                memcpy(c->up_blocks_key, p.rec_key, sizeof p.rec_key);
                c->cp_nblocks = nblk;
            }
            if (p.use_toep) {   // kernel 2f operands: lattice cell -> element map, Toeplitz weight fragments, the column's store targets
                c->toep_saw = p.toep.saw;
                c->toep_nsa = p.toep.nsa;
                if (c->toep_nsa > 16) return fail(c, OLX_ESTATE, "kernel 2f: more than 16 super-block columns");      // (ks_mask holds 2 bits per column)
                c->toep_ksmask = p.toep.ks_mask;
                for (int q = 0; q < 4; ++q) c->toep_targets[q] = p.tiles[0][0].tgt[q];
                { int rc = c->d_cell.reserve(c, c->lat.cell.size()); if (rc) return rc; }
                HIPCHK(c, hipMemcpy(c->d_cell, c->lat.cell.data(), sizeof(int) * c->lat.cell.size(), hipMemcpyHostToDevice));
                c->afrag_half = (size_t)p.mp.n_tiles * c->toep_nsa * 8 * c->lat.nsb * 4 * 64;
                { int rc = c->d_afrag.reserve(c, 2 * c->afrag_half); if (rc) return rc; }      // (a second set in the other arithmetic for a launch split at fp8_kcut)
            }
        }
    } else if (!p.perm.empty()) {      // kernel 2b
        int rc = upload_if_changed(c, c->d_perm, c->up_perm, p.perm);
        if (!rc) rc = c->d_tab.reserve(c, (size_t)((F + c->nf - 1) / c->nf) * n * (SH_HEAD + 2 * c->dx * c->dy * c->nf));  // never trust the plan-time bound
        if (rc) return rc;
    }
    c->variant = p.variant;
    c->configured_version = c->steer_version;
    return OLX_OK;
}

// Operands and block records of a kernel 2e / 2f / 2g launch: all of them -- or, for a launch split at fp8_kcut, the plane blocks from the
// cut on (e4m3 corrections: records [0, cp_nfar)) and with `below` the blocks under it (fp16 x 3: the rest, their operands a half further on)
static LatticePart lattice_part(const olx_ctx* c, bool below) {
    if (below) return {c->d_bfrag + c->bfrag_half, c->d_afrag + c->afrag_half, c->d_cpblocks + c->cp_nfar, c->cp_nblocks - c->cp_nfar, false};
    const bool split = c->fp8corr && c->cp_nfar < c->cp_nblocks;
    return {c->d_bfrag, c->d_afrag, c->d_cpblocks, split ? c->cp_nfar : c->cp_nblocks, c->fp8corr};
}

static int pack_if_needed(olx_ctx* c) {
    if (c->packed_version == c->steer_version) return OLX_OK;
    if (c->configured_version != c->steer_version) { int rc = configure_variant(c); if (rc) return rc; }
    const double lambda = c->c / c->freq;
    if (c->hetero) {
        olx_pack_hetero(c);
    } else if (c->use_mfma) {
        const double ox = c->mx == 2 ? c->grid.origin[0] + 0.5 * (c->grid.n[0] - 1) * c->grid.spacing[0] : c->grid.origin[0];
        const double oy = c->my == 2 ? c->grid.origin[1] + 0.5 * (c->grid.n[1] - 1) * c->grid.spacing[1] : c->grid.origin[1];
        dim3 g(c->mp.n_el_pad / 16, c->mp.n_tiles, c->nt);
        hipLaunchKernelGGL(mfma_pack_k, g, dim3(64), 0, c->stream, c->d_pos, c->d_area, c->n_el, c->mp.n_el_pad, c->d_delays,
                           c->d_apod, c->d_perm, ox, oy, c->grid.origin[2], c->freq, c->mfma_wscale, c->freq / c->c,
                           c->plan_foci, c->d_colinfo, c->use_lattice ? c->d_slot : nullptr,
                           (c->use_lattice && c->use_coset && c->fp8corr) ? 1 : 0, (c->use_lattice && c->use_cosetp) ? 1 : 0,
                           c->near ? (c->mx == 2 ? 0.5 : 1.0) * c->grid.spacing[0] : 0.0, (c->my == 2 ? 0.5 : 1.0) * c->grid.spacing[1], c->grid.spacing[2], c->d_coords, c->d_bfrag);
        if (c->use_lattice && c->use_toep) olx_pack_toep(c, lattice_part(c, false));
        if (c->use_lattice && c->use_coset && c->fp8corr && c->cp_nfar < c->cp_nblocks) {   // a launch split at fp8_kcut: the fp16 operands of the plane blocks below the cut
            hipLaunchKernelGGL(mfma_pack_k, g, dim3(64), 0, c->stream, c->d_pos, c->d_area, c->n_el, c->mp.n_el_pad, c->d_delays,
                               c->d_apod, c->d_perm, ox, oy, c->grid.origin[2], c->freq, c->mfma_wscale, c->freq / c->c,
                               c->plan_foci, c->d_colinfo, c->d_slot, 0, c->use_cosetp ? 1 : 0, 1.0, 1.0, 1.0, c->d_coords, c->d_bfrag + c->bfrag_half);
            if (c->use_toep) olx_pack_toep(c, lattice_part(c, true));
        }
    } else if (c->mx * c->my * c->nf == 1) {
        dim3 g((c->n_el + 127) / 128, c->plan_foci);
        // split coordinates where a voxel comes within a wavelength of an element (always with the clamp), and for the modifier kernel (field_accum_dir_k)
        c->tab_split = c->near || c->modifier();
        hipLaunchKernelGGL(steer_pack_k, g, dim3(128), 0, c->stream, c->d_pos, c->d_area, c->n_el, c->d_delays,
                           c->d_apod, c->grid.origin[0], c->grid.origin[1], c->grid.origin[2], c->freq,
                           c->p0_pa / lambda, c->freq / c->c, nullptr, nullptr, c->tab_split ? c->grid.spacing[0] : 0.0, c->grid.spacing[1], c->grid.spacing[2], c->d_tab);
        if (c->directivity) {   // frame table: { ex, pi w / lambda (as revolutions: w / (2 lambda)) | ey = n x ex, l / (2 lambda) } per element
            const int n = c->n_el;
            std::vector<float> t2((size_t)n * 8);
            for (int e = 0; e < n; ++e) {
                const double* x = &c->h_xaxis[3 * (size_t)e]; const double* nr = &c->h_nrm[3 * (size_t)e];
                const double y[3] = {nr[1] * x[2] - nr[2] * x[1], nr[2] * x[0] - nr[0] * x[2], nr[0] * x[1] - nr[1] * x[0]};
                float* t = &t2[(size_t)e * 8];
                t[0] = (float)x[0]; t[1] = (float)x[1]; t[2] = (float)x[2]; t[3] = (float)(0.5 * c->h_size[2 * (size_t)e] / lambda);
                t[4] = (float)y[0]; t[5] = (float)y[1]; t[6] = (float)y[2]; t[7] = (float)(0.5 * c->h_size[2 * (size_t)e + 1] / lambda);
            }
            { int rc = c->d_tab2.reserve(c, t2.size()); if (rc) return rc; }
            HIPCHK(c, hipMemcpyAsync(c->d_tab2, t2.data(), sizeof(float) * t2.size(), hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));   // t2 lives on this stack frame
        }
    } else {
        // mirrored axes: table coordinates relative to the grid centre plane
        const double ox = c->mx == 2 ? c->grid.origin[0] + 0.5 * (c->grid.n[0] - 1) * c->grid.spacing[0] : c->grid.origin[0];
        const double oy = c->my == 2 ? c->grid.origin[1] + 0.5 * (c->grid.n[1] - 1) * c->grid.spacing[1] : c->grid.origin[1];
        const int tiles = (c->plan_foci + c->nf - 1) / c->nf;
        dim3 g((c->n_el + 127) / 128, tiles);
        hipLaunchKernelGGL(steer_pack_shared_k, g, dim3(128), 0, c->stream, c->d_pos, c->d_area, c->n_el, c->d_delays,
                           c->d_apod, c->d_perm, ox, oy, c->grid.origin[2], c->freq, c->p0_pa / lambda, c->freq / c->c,
                           c->plan_foci, c->nf, c->dx * c->dy, c->near ? (c->mx == 2 ? 0.5 : 1.0) * c->grid.spacing[0] : 0.0, (c->my == 2 ? 0.5 : 1.0) * c->grid.spacing[1], c->grid.spacing[2], c->d_tab);
    }
    HIPCHK(c, hipGetLastError());
    c->packed_version = c->steer_version;
    return OLX_OK;
}

}  // extern "C"

// olx_field_plan of a pulsed model (olx_field_pulse, kernel 2p): whole grid, homogeneous medium, one launch of field_pulse_k
static int plan_pulse(olx_ctx* c, const olx_grid* g, const olx_slab* slab, int n_foci, double freq, double cs, double rho, double p0_pa,
                      unsigned flags) {
    if (flags & ~(OLX_OUT_PMAG | OLX_OUT_INTENSITY | OLX_OUT_PMAX | OLX_OUT_PII | OLX_FIELD_FP8_CORRECTION | OLX_FIELD_FP16_CORRECTION))
        return fail(c, OLX_EINVAL, "olx_field_plan: a pulsed plan (olx_field_pulse) takes OLX_OUT_PMAG / OLX_OUT_INTENSITY / OLX_OUT_PMAX / OLX_OUT_PII only "
                    "(no complex output, no OLX_FIELD_DIRECTIVITY), flags 0x%x", flags);
    if (slab && !(slab->x_begin == 0 && slab->x_count == g->n[0]))
        return fail(c, OLX_EINVAL, "olx_field_plan: a pulsed plan (olx_field_pulse) covers the whole grid: no slab");
    if (c->comm_active()) return fail(c, OLX_ESTATE, "olx_field_plan: a pulsed plan (olx_field_pulse) has no multi-GPU path: destroy the communicator first");
    const long long vox = (long long)g->n[0] * g->n[1] * g->n[2];
    if (vox > (1ll << 31) * 4) return fail(c, OLX_EINVAL, "olx_field_plan: grid too large for a pulsed plan");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t total = (size_t)vox * n_foci;
    c->grid = *g; c->slab = olx_slab{0, g->n[0]}; c->plan_foci = n_foci; c->hetero = false; c->marched = false;
    c->agg_local = -1; c->agg_total = 0;
    c->freq = freq; c->c = cs; c->rho = rho; c->p0_pa = p0_pa; c->flags = flags; c->plan_absorb = c->absorb_np_m;
    c->directivity = false; c->nbuf = 1; c->cur = 0;
    const size_t fn = (size_t)n_foci * c->n_el;
    pii_regrid(c, vox);
    c->derive_i = false; c->inten_live = false;      // (a pulsed plan stores its intensity)
    int rc = reserve_outputs(c, total, 1, (flags & OLX_OUT_INTENSITY) != 0, false, false);
    if (!rc && (flags & OLX_OUT_PMAX)) rc = c->d_pmax.reserve(c, total);
    if (!rc && (flags & OLX_OUT_PII)) rc = c->d_pii.reserve(c, total);
    if (!rc) rc = c->d_ptab.reserve(c, fn);
    if (!rc) rc = c->d_pw.reserve(c, fn);
    if (rc) return rc;
    // drive impulse responses (olx_field_pulse_response): class table and row table as one int buffer, gamma in fp64 -> float2, of THIS plan's f0 dt
    const int n_resp = c->resp_row.empty() ? 0 : (int)c->resp_row.size() - 1;
    if (n_resp > 0) {
        if ((int)c->resp_cls.size() != c->n_el) return fail(c, OLX_ESTATE, "olx_field_plan: the impulse responses belong to another element table");
        std::vector<int> tab(c->resp_cls);
        tab.insert(tab.end(), c->resp_row.begin(), c->resp_row.end());
        const int n_taps = c->resp_row[n_resp];
        std::vector<float> gam(2 * (size_t)n_taps);
        int m_max = 1;
        for (int r = 0; r < n_resp; ++r) {
            m_max = std::max(m_max, c->resp_row[r + 1] - c->resp_row[r]);
            for (int g = c->resp_row[r]; g < c->resp_row[r + 1]; ++g) {
                double cyc = freq * c->pulse_dt * (double)(g - c->resp_row[r]);
                cyc -= std::floor(cyc);
                gam[2 * (size_t)g] = (float)(c->resp_taps[g] * std::cos(2.0 * M_PI * cyc));
                gam[2 * (size_t)g + 1] = (float)(-c->resp_taps[g] * std::sin(2.0 * M_PI * cyc));
            }
        }
        rc = c->d_presp_tab.reserve(c, tab.size());
        if (!rc) rc = c->d_presp_gam.reserve(c, gam.size());
        if (rc) return rc;
        HIPCHK(c, hipMemcpy(c->d_presp_tab, tab.data(), sizeof(int) * tab.size(), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(c->d_presp_gam, gam.data(), sizeof(float) * gam.size(), hipMemcpyHostToDevice));
        c->presp_taps = n_taps; c->presp_hist = m_max - 1;
    }
    c->presp_classes = n_resp;
    // (the scans -- aggregate, scale, analysis -- read the volume shape from fp)
    FieldParams& F = c->fp;
    F.nx = g->n[0]; F.ny = g->n[1]; F.nz = g->n[2]; F.n_el = c->n_el; F.x_begin = 0; F.vox = vox;
    F.flags = (flags & 3u) | OLX_OUT_PMAG; F.inten_scale = (float)(1e-4 / (2.0 * rho * cs));
    PulseParams& P = c->pulse;
    const double dt = c->pulse_dt;
    c->pulse_plan_dt = dt;
    P.n_el = c->n_el; P.n_foci = n_foci; P.n_t = c->pulse_nt; P.ny = g->n[1]; P.nz = g->n[2];
    P.ox = g->origin[0]; P.oy = g->origin[1]; P.oz = g->origin[2];
    P.hx = g->spacing[0]; P.hy = g->spacing[1]; P.hz = g->spacing[2];
    P.dmin = 0.5 * std::min({g->spacing[0], g->spacing[1], g->spacing[2]});
    P.inv_cdt = 1.0 / (cs * dt);
    P.tdt = c->pulse_cycles / (freq * dt);
    P.f0dt = freq * dt;
    P.dmin_f = (float)P.dmin; P.inv_cdt_f = (float)P.inv_cdt;
    P.absorb = (float)c->absorb_np_m;
    P.rot_c = (float)std::cos(2.0 * M_PI * P.f0dt); P.rot_s = (float)std::sin(2.0 * M_PI * P.f0dt);
    P.inten_scale = F.inten_scale;
    P.pii_scale = (float)(1e-4 * dt / (rho * cs));
    P.vox = vox;
    c->pulsed = true; c->pmax_live = false; c->agg_pmax_valid = false; c->pii_live = false;
    c->pulse_med = false;      // (olx_field_pulse_medium belongs to the plan it was called on)
    char nm[128];
    snprintf(nm, sizeof nm, "field_pulse_k (pulsed: %d samples, %.4g samples per burst)", c->pulse_nt, P.tdt);
    c->variant = nm;
    if (c->presp_classes > 0) {
        snprintf(nm, sizeof nm, "; response: %d classes, %d taps", c->presp_classes, c->presp_hist + 1);
        c->variant += nm;
    }
    c->packed_version = ~0ull;
    c->planned = true; c->uploaded = false;
    return OLX_OK;
}

extern "C" {

int olx_field_plan(olx_ctx* c, const olx_grid* g, const olx_slab* slab, int n_foci, double freq, double cs,
                   double rho, double p0_pa, unsigned flags) {
    if (!c) return OLX_EINVAL;
    if (c->n_el <= 0) return fail(c, OLX_ESTATE, "olx_field_plan: call olx_set_elements first");
    if (c->n_foci <= 0) return fail(c, OLX_ESTATE, "olx_field_plan: no steering table (olx_bf_solve / olx_set_steering)");
    if (!g) return fail(c, OLX_EINVAL, "olx_field_plan: null grid");
    if (n_foci != c->n_foci) return fail(c, OLX_EINVAL, "olx_field_plan: n_foci %d != steering table foci %d", n_foci, c->n_foci);
    for (int a = 0; a < 3; ++a)
        if (g->n[a] < 1 || !(g->spacing[a] > 0)) return fail(c, OLX_EINVAL, "olx_field_plan: bad grid axis %d", a);
    if (!(freq > 0) || !(cs > 0) || !(rho > 0)) return fail(c, OLX_EINVAL, "olx_field_plan: freq, c, rho must be > 0");
    if (!(flags & (OLX_OUT_PMAG | OLX_OUT_INTENSITY | OLX_OUT_COMPLEX))) return fail(c, OLX_EINVAL, "olx_field_plan: no outputs selected");
    if (c->pulse_nt > 0) return plan_pulse(c, g, slab, n_foci, freq, cs, rho, p0_pa, flags);
    if (flags & OLX_OUT_PMAX) return fail(c, OLX_EINVAL, "olx_field_plan: OLX_OUT_PMAX needs a pulsed plan (olx_field_pulse)");
    if (flags & OLX_OUT_PII) return fail(c, OLX_EINVAL, "olx_field_plan: OLX_OUT_PII needs a pulsed plan (olx_field_pulse)");
    if (flags & ~(OLX_OUT_PMAG | OLX_OUT_INTENSITY | OLX_OUT_COMPLEX | OLX_FIELD_FP8_CORRECTION | OLX_FIELD_FP16_CORRECTION | OLX_FIELD_DIRECTIVITY)) return fail(c, OLX_EINVAL, "olx_field_plan: unknown flag bits 0x%x", flags);
    if ((flags & OLX_FIELD_DIRECTIVITY) && c->h_xaxis.size() != 3 * (size_t)c->n_el)
        return fail(c, OLX_ESTATE, "olx_field_plan: OLX_FIELD_DIRECTIVITY needs olx_set_element_apertures");
    olx_slab s{0, g->n[0]};
    if (slab) s = *slab;
    if (s.x_begin < 0 || s.x_count < 1 || s.x_begin + s.x_count > g->n[0]) return fail(c, OLX_EINVAL, "olx_field_plan: slab outside grid");
    HIPCHK(c, hipSetDevice(c->device));
    {   // Re-planning the SAME launch (same grid, slab, foci count, medium constants, flags, element table, family pins): everything
        // derived below is still valid -- an interactive caller re-plans per target while only the steering changes.  The steering-
        // dependent part (configure_variant + packing) is redone at the next launch anyway when the table changed.
        std::string env;   // the developer switches the plan below reads
        for (const char* name : {"OLX_FIELD_VARIANT", "OLX_FP8_CORRECTION", "OLX_EXP_TOEP_SAW", "OLX_EXP_TOEP_NM", "OLX_EXP_KGRP", "OLX_INTENSITY_STORED", "OLX_EXP_CP_NOREUSE", "OLX_EXP_CP_NOFILLAHEAD", "OLX_EXP_CP_NOSORT"}) { const char* e = getenv(name); env += e ? e : ""; env += '|'; }
        const bool same = c->planned && !c->uploaded && !c->hetero && !c->pulsed && memcmp(&c->grid, g, sizeof *g) == 0 && c->slab.x_begin == s.x_begin &&
                          c->slab.x_count == s.x_count && c->plan_foci == n_foci && c->freq == freq && c->c == cs && c->rho == rho &&
                          c->p0_pa == p0_pa && c->flags == flags && c->plan_absorb == c->absorb_np_m && c->nbuf == (c->comm_active() ? olx_ctx::NBUF : 1) && c->plan_env == env;
        c->plan_env = env;
        if (same) {
            c->agg_local = -1; c->agg_total = 0;
            if (c->packed_version != c->steer_version) return configure_variant(c);   // (names the variant for olx_field_variant; packed at launch)
            return OLX_OK;
        }
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->grid = *g; c->slab = s; c->plan_foci = n_foci; c->hetero = false;
    c->pulse_med = false;
    c->pulsed = false; c->pmax_live = false; c->agg_pmax_valid = false; c->pii_live = false;
    c->agg_local = -1; c->agg_total = 0;   // aggregate over all planned foci unless olx_field_aggregate_counts says otherwise
    c->freq = freq; c->c = cs; c->rho = rho; c->p0_pa = p0_pa; c->flags = flags; c->plan_absorb = c->absorb_np_m;
    const long long vox = (long long)s.x_count * g->n[1] * g->n[2];
    pii_regrid(c, vox);
    const size_t total = (size_t)vox * n_foci;
    c->nbuf = c->comm_active() ? olx_ctx::NBUF : 1;
    // outputs (|p| is always materialised: aggregate / allgather consume it)
    // Intensity: derived from |p| by its readers unless pinned to the stored form (every homogeneous kernel 2 variant drops the store when its own
    // flags say so, so the mode does not depend on the variant the steering selects later; olx_field_set_medium switches the plan back to stored)
    { const char* pin = getenv("OLX_INTENSITY_STORED"); c->derive_i = (flags & OLX_OUT_INTENSITY) && !(pin && *pin && strcmp(pin, "0") != 0); }
    c->inten_live = false;
    { int rc = reserve_outputs(c, total, c->nbuf, (flags & OLX_OUT_INTENSITY) && !c->derive_i, (flags & OLX_OUT_COMPLEX) != 0, true); if (rc) return rc; }
    if (c->derive_i) c->d_inten.release();       // (volumes of an earlier, stored plan)
    { int rc = c->d_tab.reserve(c, (size_t)n_foci * c->n_el * TAB_STRIDE); if (rc) return rc; }
    // kernel parameters.  Table origin = grid origin; slab start expressed relative to it.
    FieldParams& P = c->fp;
    P.nx = s.x_count; P.ny = g->n[1]; P.nz = g->n[2]; P.n_el = c->n_el;
    P.x_begin = s.x_begin;
    const double rev = freq / cs;  // kernel lengths are in wavelengths
    P.hx = (float)(g->spacing[0] * rev); P.hy = (float)(g->spacing[1] * rev); P.hz = (float)(g->spacing[2] * rev);
    const double dmin = 0.5 * std::min({g->spacing[0], g->spacing[1], g->spacing[2]});
    P.dmin2 = (float)(dmin * dmin * rev * rev);
    P.inten_scale = (float)(1e-4 / (2.0 * rho * cs));
    P.vox = vox; P.flags = ((flags & 7u) | OLX_OUT_PMAG) & ~(c->derive_i ? (unsigned)OLX_OUT_INTENSITY : 0u);
    c->directivity = (flags & OLX_FIELD_DIRECTIVITY) != 0;
    // variant decisions from host copies (exact, fp64)
    const int n = c->n_el;
    const double* hz = c->h_pos.data() + 2 * (size_t)n;
    c->flat = true;
    for (int e = 1; e < n; ++e) if (hz[e] != hz[0]) { c->flat = false; break; }
    P.flat_ez = (float)((hz[0] - g->origin[2]) * rev);
    { const double kz = std::rint((hz[0] - g->origin[2]) / g->spacing[2]); P.flat_kz = (float)kz; P.flat_fz = (float)(((hz[0] - g->origin[2]) - kz * g->spacing[2]) * rev); }
    // clamp needed iff some element lies within dmin (+ fp32 slack) of the slab's bounding box
    double lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
        const int b = (a == 0) ? s.x_begin : 0;
        const int cnt = (a == 0) ? s.x_count : g->n[a];
        lo[a] = g->origin[a] + b * g->spacing[a];
        hi[a] = g->origin[a] + (b + cnt - 1) * g->spacing[a];
    }
    c->clamp = false;
    const double guard = 2.0 * dmin;
    double min_d2 = 1e300;
    for (int e = 0; e < n; ++e) {
        double d2 = 0;
        for (int a = 0; a < 3; ++a) {
            const double p = c->h_pos[(size_t)a * n + e];
            const double d = p < lo[a] ? lo[a] - p : (p > hi[a] ? p - hi[a] : 0.0);
            d2 += d * d;
        }
        min_d2 = std::min(min_d2, d2);
        if (d2 < guard * guard) c->clamp = true;
    }
    c->min_dist = c->clamp ? dmin : std::sqrt(min_d2);  // lower bound of any voxel-element distance [m]
    // a voxel within a QUARTER wavelength of an element: the general kernels (2a / 2b / 2c) then work from index differences (k_accum.hip) -- absolute fp32
    // coordinates of ~ 10 wavelengths lose 1e-6 wavelengths, i.e. up to 4e-6 of a term at a quarter wavelength and 1.5e-5 at the clamp distance of a 0.25 mm grid
    c->near = c->clamp || c->min_dist < 0.25 * cs / freq;
    detect_lattice(c, lo, hi, dmin);
    c->nf_s2.clear();     // near-field sums of the e4m3 error bound: derived lazily by configure_variant (olxplan::fp8_first_plane)
    // ---- shared-geometry variant: mirror folds (element set symmetric about the grid centre planes)
    auto mirror_perm = [&](int axis, std::vector<int>& perm) -> bool {
        const double ctr = g->origin[axis] + 0.5 * (g->n[axis] - 1) * g->spacing[axis];
        const double tol = 1e-12;
        perm.assign(n, -1);
        std::vector<char> used(n, 0);
        for (int e = 0; e < n; ++e) {
            const double want = 2.0 * ctr - c->h_pos[(size_t)axis * n + e];
            int hit = -1;
            for (int o = 0; o < n && hit < 0; ++o) {
                if (used[o] || std::fabs(c->h_pos[(size_t)axis * n + o] - want) > tol) continue;
                bool same = true;
                for (int a = 0; a < 3; ++a)
                    if (a != axis && std::fabs(c->h_pos[(size_t)a * n + o] - c->h_pos[(size_t)a * n + e]) > tol) same = false;
                if (same) hit = o;
            }
            if (hit < 0) return false;
            used[hit] = 1; perm[e] = hit;
        }
        return true;
    };
    const bool whole_x = (s.x_begin == 0 && s.x_count == g->n[0]);
    const char* force = getenv("OLX_FIELD_VARIANT");  // general | shared | mfma | lattice: pin a kernel family (A/B measurements)
    c->force_kind = !force ? 0 : !strcmp(force, "general") ? 1 : !strcmp(force, "shared") ? 2 : !strcmp(force, "mfma") ? 3 : (!strcmp(force, "lattice") || !strcmp(force, "lattice2d")) ? 4 : 0;
    // piston directivity: for a flat array of equal, axis-aligned elements D_e depends on the (voxel - element) offset only and folds
    // into the lattice kernels' geometry tables (their DIR instantiations); any other array keeps the exact per-pair kernel 2a-d
    c->dir_lattice = false;
    P.absorb_l2 = (float)(c->absorb_np_m * (cs / freq) * 1.4426950408889634);       // kernel 2a-d: exp(-a d) = exp2(-a lambda log2(e) d'), d' [wavelengths]
    if (c->modifier() && !(flags & OLX_OUT_COMPLEX) && c->flat) {
        bool ok = !c->directivity || (c->h_xaxis.size() == 3 * (size_t)n && c->h_size.size() == 2 * (size_t)n);
        for (int e = 0; c->directivity && ok && e < n; ++e) {
            const double* xa = &c->h_xaxis[3 * (size_t)e]; const double* nr = &c->h_nrm[3 * (size_t)e];
            if (std::fabs(std::fabs(xa[0]) - 1.0) > 1e-12 || std::fabs(xa[1]) > 1e-12 || std::fabs(xa[2]) > 1e-12) ok = false;
            if (std::fabs(std::fabs(nr[2]) - 1.0) > 1e-12) ok = false;
            if (c->h_size[2 * (size_t)e] != c->h_size[0] || c->h_size[2 * (size_t)e + 1] != c->h_size[1]) ok = false;
        }
        c->dir_lattice = ok;
    }
    c->allow_shared = c->force_kind != 1 && c->force_kind != 5 && (!c->modifier() || c->dir_lattice);
    c->mx = (c->allow_shared && whole_x && g->n[0] >= 2 && n <= 8192 && mirror_perm(0, c->h_px)) ? 2 : 1;
    c->my = (c->allow_shared && g->n[1] >= 2 && n <= 8192 && mirror_perm(1, c->h_py)) ? 2 : 1;
    {   // worst-case kernel-2a/2b table over every (dx, dy, nf) the steering may select later: tiles = ceil(F / nf)
        // entries of 4 + 2 dx dy nf <= 20 floats, i.e. at most 12 F + 20 floats per element (the last tile is padded)
        int rc = c->d_tab.reserve(c, ((size_t)n_foci * 12 + 24) * n);
        if (c->d_perm.capacity() < (size_t)4 * n) c->up_perm.clear();     // (a new block holds no uploaded permutation)
        if (!rc) rc = c->d_perm.reserve(c, (size_t)4 * n);
        if (rc) return rc;
    }
    SharedParams& S = c->sp;
    S.nx = P.nx; S.ny = P.ny; S.nz = P.nz; S.n_el = n; S.x_begin = s.x_begin; S.n_foci = n_foci;
    S.hx = P.hx; S.hy = P.hy; S.hz = P.hz; S.dmin2 = P.dmin2;
    S.inten_scale = P.inten_scale; S.flat_ez = P.flat_ez; S.flat_kz = P.flat_kz; S.flat_fz = P.flat_fz; S.vox = P.vox; S.flags = P.flags;
    c->dx = c->mx; c->dy = c->my; c->nf = 1;
    char nm[96] = "(steering-dependent)";
    c->variant = nm;
    c->packed_version = ~0ull;
    c->planned = true; c->uploaded = false;
    c->cur = 0;
    return configure_variant(c);  // provisional (re-evaluated when the steering table changes)
}

}  // extern "C"

extern "C" {

int olx_field_launch(olx_ctx* c) {
    if (!c) return OLX_EINVAL;
    if (!c->planned) return fail(c, OLX_ESTATE, "olx_field_launch: call olx_field_plan first");
    if (c->uploaded) return fail(c, OLX_ESTATE, "olx_field_launch: resident volumes were uploaded, not planned");
    if (c->n_foci != c->plan_foci) return fail(c, OLX_ESTATE, "olx_field_launch: steering table changed shape since plan");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->pulsed) {     // kernel 2p: its own table from the steering, no variant packing
        if (c->flags & OLX_OUT_PMAX) c->pmax_live = false;
        c->agg_pmax_valid = false; c->pii_live = false; c->pii_w_valid = false; c->pii_max_valid = false;
        const bool prof = c->prof_on && (size_t)(2 * c->prof_n + 1) < c->prof_ev.size();
        if (prof) HIPCHK(c, hipEventRecord(c->prof_ev[2 * c->prof_n], c->stream));
        if (c->pulse_med) olx_launch_pulse_med(c, c->d_pmag[0]); else olx_launch_pulse(c, c->d_pmag[0]);
        HIPCHK(c, hipGetLastError());
        if (prof) { HIPCHK(c, hipEventRecord(c->prof_ev[2 * c->prof_n + 1], c->stream)); c->prof_n++; }
        c->pmax_live = (c->flags & OLX_OUT_PMAX) != 0;
        c->pii_live = (c->flags & OLX_OUT_PII) != 0; c->pii_foci = c->plan_foci;
        c->cur = 0;
        return OLX_OK;
    }
    int rc = pack_if_needed(c);
    if (rc) return rc;
    const int b = (c->nbuf == 2) ? (c->cur ^ 1) : 0;
    if (c->gather_pending[b]) {  // the gather that read this buffer must be done before we overwrite it
        if (c->p2p) { rc = olx_p2p_before_overwrite(c, b); if (rc) { c->gather_pending[b] = false; return rc; } }   // ... on EVERY rank that pulls from it
        else HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_gather[b], 0));
        c->gather_pending[b] = false;
    }
    float* pm = c->d_pmag[b];
    c->inten_live = false;
    const bool prof = c->prof_on && (size_t)(2 * c->prof_n + 1) < c->prof_ev.size();
    if (prof) HIPCHK(c, hipEventRecord(c->prof_ev[2 * c->prof_n], c->stream));
    if (c->hetero) { if (c->marched) olx_launch_hmarch(c, pm); else olx_launch_hetero(c, pm); }
    else if (c->use_mfma) {
        if (!c->use_lattice) olx_launch_mfma(c, pm);
        else if (c->use_coset) {
            auto go = [&](const LatticePart& q) { if (c->use_toep) olx_launch_toep(c, q, pm); else if (c->use_cosetp) olx_launch_cosetp(c, q, pm); else olx_launch_coset(c, q, pm); };
            if (c->fp8corr && c->cp_nfar < c->cp_nblocks) {   // split at fp8_kcut: e4m3 corrections for the plane blocks from the cut on, three fp16 products below it
                if (c->cp_nfar) go(lattice_part(c, false));
                go(lattice_part(c, true));
            } else go(lattice_part(c, false));
        }
        else olx_launch_lattice(c, pm);
    }
    else if (c->mx * c->my * c->nf > 1) {
        if (!olx_launch_shared(c, pm)) return fail(c, OLX_ESTATE, "olx_field_launch: no kernel for variant %s", c->variant.c_str());
    } else if (c->modifier()) olx_launch_accum_dir(c, pm);
    else olx_launch_accum(c, pm);
    HIPCHK(c, hipGetLastError());
    if (prof) { HIPCHK(c, hipEventRecord(c->prof_ev[2 * c->prof_n + 1], c->stream)); c->prof_n++; }
    c->cur = b;
    return OLX_OK;
}

int olx_profile_begin(olx_ctx* c, int max_launches) {
    if (!c) return OLX_EINVAL;
    if (max_launches < 1 || max_launches > (1 << 20)) return fail(c, OLX_EINVAL, "olx_profile_begin: bad max_launches");
    HIPCHK(c, hipSetDevice(c->device));
    for (auto e : c->prof_ev) hipEventDestroy(e);
    c->prof_ev.assign(2 * (size_t)max_launches, nullptr);
    for (auto& e : c->prof_ev) HIPCHK(c, hipEventCreate(&e));
    c->prof_n = 0; c->prof_on = true;
    return OLX_OK;
}

int olx_profile_end(olx_ctx* c, float* ms_each, int capacity, int* n_recorded) {
    if (!c) return OLX_EINVAL;
    if (!ms_each || !n_recorded || capacity < 0) return fail(c, OLX_EINVAL, "olx_profile_end: null output");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int n = std::min(c->prof_n, capacity);
    for (int i = 0; i < n; ++i) HIPCHK(c, hipEventElapsedTime(&ms_each[i], c->prof_ev[2 * i], c->prof_ev[2 * i + 1]));
    *n_recorded = n;
    for (auto e : c->prof_ev) hipEventDestroy(e);
    c->prof_ev.clear(); c->prof_n = 0; c->prof_on = false;
    return OLX_OK;
}

}  // extern "C"

// Device -> caller-owned host memory.  The caller's arrays are ordinary pageable NumPy memory (ownership contract of the
// seam: fresh, writable, caller-owned -- SURVEY 8(b)); a plain hipMemcpy of such memory is staged by the runtime through
// a small pinned buffer (~25 GB/s, and it touches every destination page from ONE thread).  Modes (OLX_FETCH_MODE, for
// A/B measurements; default "staged"):
//   pageable  hipMemcpyAsync straight into the caller's pages (the round-1 path)
//   register  hipHostRegister the destination, one DMA, unregister (pinning walks / faults the pages in the kernel)
//   staged    the transfer is cut into one contiguous part per worker thread (OLX_FETCH_THREADS, default 8); each worker
//             streams its part through its own two pinned chunks on its own stream -- DMA of chunk i+1 overlaps the
//             copy-out of chunk i -- so the first touch of the destination pages and the copy-out run on several cores
struct FetchLane {                 // one per worker thread: its own stream and two pinned chunks
    static constexpr size_t CAPACITY = (size_t)8 << 20;   // bytes per pinned buffer; a transfer uses pieces of <= this
    hipStream_t stream = nullptr;
    void* buf[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool ok = false;
    void release() {
        for (int i = 0; i < 2; ++i) {
            if (ev[i]) hipEventDestroy(ev[i]);
            if (buf[i]) hipHostFree(buf[i]);
            ev[i] = nullptr; buf[i] = nullptr;
        }
        if (stream) hipStreamDestroy(stream);
        stream = nullptr; ok = false;
    }
    bool init() {                  // complete or not at all: a partial failure leaves nothing behind and is retried next time
        if (ok) return true;
        release();
        bool good = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) == hipSuccess;
        for (int i = 0; good && i < 2; ++i)
            good = hipHostMalloc(&buf[i], CAPACITY, hipHostMallocDefault) == hipSuccess &&
                   hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) == hipSuccess;
        if (!good) { (void)hipGetLastError(); release(); return false; }
        return ok = true;
    }
};
static constexpr int FETCH_MAX_THREADS = 32;
// The lanes belong to the CONTEXT (olx_ctx::fetch_lanes, freed by olx_ctx_destroy): two contexts on one device fetching from two
// threads never share pinned chunks (ctypes releases the GIL; the contract is one caller thread per context).
static FetchLane* ctx_fetch_lanes(olx_ctx* c) {
    if (!c->fetch_lanes) c->fetch_lanes = new FetchLane[FETCH_MAX_THREADS];
    return c->fetch_lanes;
}
static void free_fetch_lanes(olx_ctx* c) {
    if (!c->fetch_lanes) return;
    for (int t = 0; t < FETCH_MAX_THREADS; ++t) c->fetch_lanes[t].release();
    delete[] c->fetch_lanes;
    c->fetch_lanes = nullptr;
}

// Worker t moves bytes [lo, hi) of the transfer: DMA of chunk i+1 into its second pinned buffer is in flight while it
// copies chunk i into the destination (first touch of those destination pages happens on this thread).
static hipError_t fetch_lane_run(int device, FetchLane& L, char* dst, const char* src, size_t lo, size_t hi, size_t chunk) {
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return e;
    const size_t n = (hi - lo + chunk - 1) / chunk;
    auto issue = [&](size_t i) {
        const size_t off = lo + i * chunk, cnt = std::min(chunk, hi - off);
        hipError_t r = hipMemcpyAsync(L.buf[i & 1], src + off, cnt, hipMemcpyDeviceToHost, L.stream);
        return r != hipSuccess ? r : hipEventRecord(L.ev[i & 1], L.stream);
    };
    if (n) { e = issue(0); if (e != hipSuccess) return e; }
    for (size_t i = 0; i < n; ++i) {
        if (i + 1 < n) { e = issue(i + 1); if (e != hipSuccess) return e; }
        e = hipEventSynchronize(L.ev[i & 1]);
        if (e != hipSuccess) return e;
        const size_t off = lo + i * chunk, cnt = std::min(chunk, hi - off);
        memcpy(dst + off, L.buf[i & 1], cnt);
    }
    return hipSuccess;
}

static int fetch_to_host(olx_ctx* c, void* dst, const void* src, size_t bytes) {
    const char* mode_env = getenv("OLX_FETCH_MODE");
    const int mode = !mode_env ? 2 : !strcmp(mode_env, "pageable") ? 0 : !strcmp(mode_env, "register") ? 1 : 2;
    if (mode == 1 && bytes >= ((size_t)1 << 20)) {
        if (hipHostRegister(dst, bytes, hipHostRegisterDefault) == hipSuccess) {
            hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            hipHostUnregister(dst);
            if (e != hipSuccess) return fail(c, OLX_EHIP, "fetch (registered): %s", hipGetErrorString(e));
            return OLX_OK;
        }
        (void)hipGetLastError();   // fall through to the pageable copy
    }
    if (mode == 2 && bytes >= ((size_t)8 << 20)) {
        int nthr = 8;
        if (const char* t = getenv("OLX_FETCH_THREADS")) nthr = atoi(t);
        const int hw = (int)std::thread::hardware_concurrency();
        nthr = std::max(1, std::min({nthr, FETCH_MAX_THREADS, hw > 0 ? hw : 1, (int)(bytes >> 21)}));
        // piece size: every worker should see >= 4 pieces (DMA of piece i+1 behind the copy-out of piece i), 2 MB at least and the
        // pinned buffer at most -- one 67 MB volume moves in 2 MB pieces (35 GB/s; 24 in 8 MB pieces, four workers), eight volumes in
        // 8 MB pieces (46 GB/s; 43 in 2 MB pieces): tools/fetch_bench.py
        size_t chunk = std::min(FetchLane::CAPACITY, std::max((size_t)2 << 20, (bytes / nthr / 4 + 4095) & ~(size_t)4095));
        if (const char* t = getenv("OLX_FETCH_CHUNK_KB"))
            chunk = std::min(FetchLane::CAPACITY, std::max((size_t)64, (size_t)atol(t)) << 10);
        FetchLane* lanes = ctx_fetch_lanes(c);
        bool ready = true;
        for (int t = 0; t < nthr; ++t) ready = ready && lanes[t].init();
        if (ready) {
            const size_t per = ((bytes / nthr) + 4095) & ~(size_t)4095;
            std::vector<hipError_t> rc(nthr, hipSuccess);
            std::vector<std::thread> th;
            for (int t = 0; t < nthr; ++t) {
                const size_t lo = std::min(per * t, bytes), hi = t == nthr - 1 ? bytes : std::min(per * (t + 1), bytes);
                th.emplace_back([&, t, lo, hi] { rc[t] = fetch_lane_run(c->device, lanes[t], (char*)dst, (const char*)src, lo, hi, chunk); });
            }
            for (auto& t : th) t.join();
            for (int t = 0; t < nthr; ++t)
                if (rc[t] != hipSuccess) return fail(c, OLX_EHIP, "fetch (staged, worker %d): %s", t, hipGetErrorString(rc[t]));
            return OLX_OK;
        }
        (void)hipGetLastError();
    }
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return OLX_OK;
}

// The intensity of foci [first, first + count) of a deriving plan: formed from |p| one focus at a time in a one-volume scratch block, copied out from there
static int fetch_derived_intensity(olx_ctx* c, float* out, int first, int count) {
    const size_t vox = (size_t)c->fp.vox;
    { int rc = c->d_ifetch.reserve(c, vox); if (rc) return rc; }
    for (int f = first; f < first + count; ++f) {
        inten_fill(c, c->d_pmag[c->cur] + vox * f, vox, c->d_ifetch);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
        const int rc = fetch_to_host(c, out + vox * (size_t)(f - first), c->d_ifetch, sizeof(float) * vox);
        if (rc) return rc;
    }
    return OLX_OK;
}

extern "C" {

int olx_field_fetch(olx_ctx* c, int focus, float* pmag, float* intensity, float* cplx) {
    if (!c) return OLX_EINVAL;
    if (!c->planned) return fail(c, OLX_ESTATE, "olx_field_fetch: nothing planned");
    if (focus < 0 || focus >= c->plan_foci) return fail(c, OLX_EINVAL, "olx_field_fetch: focus %d out of range", focus);
    if (intensity && !(c->flags & OLX_OUT_INTENSITY)) return fail(c, OLX_ESTATE, "olx_field_fetch: intensity not planned");
    if (cplx && !(c->flags & OLX_OUT_COMPLEX)) return fail(c, OLX_ESTATE, "olx_field_fetch: complex output not planned");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t vox = (size_t)c->fp.vox, off = vox * focus;
    int rc = OLX_OK;
    if (pmag) rc = fetch_to_host(c, pmag, c->d_pmag[c->cur] + off, sizeof(float) * vox);
    if (!rc && intensity) {
        if (c->derive_i && !c->inten_live) rc = fetch_derived_intensity(c, intensity, focus, 1);
        else rc = fetch_to_host(c, intensity, c->d_inten + off, sizeof(float) * vox);
    }
    if (!rc && cplx) rc = fetch_to_host(c, cplx, c->d_cplx + 2 * off, sizeof(float) * 2 * vox);
    return rc;
}

int olx_field_fetch_all(olx_ctx* c, float* pmag, float* intensity) {
    if (!c) return OLX_EINVAL;
    if (!c->planned) return fail(c, OLX_ESTATE, "olx_field_fetch_all: nothing planned");
    if (intensity && !(c->flags & OLX_OUT_INTENSITY)) return fail(c, OLX_ESTATE, "olx_field_fetch_all: intensity not planned");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t total = (size_t)c->fp.vox * c->plan_foci;
    int rc = OLX_OK;
    if (pmag) rc = fetch_to_host(c, pmag, c->d_pmag[c->cur], sizeof(float) * total);
    if (!rc && intensity) {
        if (c->derive_i && !c->inten_live) rc = fetch_derived_intensity(c, intensity, 0, c->plan_foci);
        else rc = fetch_to_host(c, intensity, c->d_inten, sizeof(float) * total);
    }
    return rc;
}

int olx_field_fetch_pmax(olx_ctx* c, float* pmax_out) {
    if (!c) return OLX_EINVAL;
    if (!pmax_out) return fail(c, OLX_EINVAL, "olx_field_fetch_pmax: null output");
    if (!c->pmax_live) return fail(c, OLX_ESTATE, "olx_field_fetch_pmax: no p_max volumes (a launched pulsed plan with OLX_OUT_PMAX)");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return fetch_to_host(c, pmax_out, c->d_pmax, sizeof(float) * (size_t)c->fp.vox * c->plan_foci);
}

int olx_field_fetch_pii(olx_ctx* c, float* pii_out) {
    if (!c) return OLX_EINVAL;
    if (!pii_out) return fail(c, OLX_EINVAL, "olx_field_fetch_pii: null output");
    if (!c->pii_live) return fail(c, OLX_ESTATE, "olx_field_fetch_pii: no pulse intensity integrals (a launched pulsed plan with OLX_OUT_PII, or olx_pii_upload)");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return fetch_to_host(c, pii_out, c->d_pii, sizeof(float) * (size_t)c->fp.vox * c->pii_foci);
}

int olx_field_pulse_trace(olx_ctx* c, int n_points, const long long* voxels, float* trace_out) {
    if (!c) return OLX_EINVAL;
    if (!c->planned || c->uploaded || !c->pulsed) return fail(c, OLX_ESTATE, "olx_field_pulse_trace: needs a pulsed plan (olx_field_pulse, then olx_field_plan)");
    if (c->n_foci != c->plan_foci) return fail(c, OLX_ESTATE, "olx_field_pulse_trace: steering table changed shape since plan");
    if (n_points < 1 || !voxels || !trace_out) return fail(c, OLX_EINVAL, "olx_field_pulse_trace: n_points must be >= 1, voxels and trace_out not null");
    for (int i = 0; i < n_points; ++i)
        if (voxels[i] < 0 || voxels[i] >= c->pulse.vox)
            return fail(c, OLX_EINVAL, "olx_field_pulse_trace: voxel %d = %lld outside the planned grid of %lld voxels", i, voxels[i], c->pulse.vox);
    const double total_d = (double)c->plan_foci * n_points * c->pulse.n_t;
    if (total_d > (double)OLX_PULSE_TRACE_MAX_SAMPLES)
        return fail(c, OLX_EINVAL, "olx_field_pulse_trace: %g trace samples are more than OLX_PULSE_TRACE_MAX_SAMPLES (trace fewer points per call)", total_d);
    const size_t total = (size_t)c->plan_foci * n_points * c->pulse.n_t;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int rc = c->d_ptrace_vox.reserve(c, n_points);
    if (!rc) rc = c->d_ptrace.reserve(c, total);
    if (rc) return rc;
    HIPCHK(c, hipMemcpy(c->d_ptrace_vox, voxels, sizeof(long long) * n_points, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemsetAsync(c->d_ptrace, 0, sizeof(float) * total, c->stream));
    if (c->pulse_med) olx_launch_pulse_med_trace(c, n_points); else olx_launch_pulse_trace(c, n_points);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));     // (a large fetch runs on streams of its own, not ordered after this one)
    return fetch_to_host(c, trace_out, c->d_ptrace, sizeof(float) * total);
}

// ---- kernel 4: steering map (DESIGN.md section 2 "Steering map") ---------------------------------------------------
// Reads the element table (and the apertures), writes buffers of its own: the plan, the steering table and every resident result stay as they are.
// What kernels 4 and 4h check and fill alike: the grid, the apodization rule and its part of SteerParams (`who` words the messages).
static int steer_params(olx_ctx* c, const char* who, const olx_grid* g, int apod_kind, double p0, double p1, SteerParams& P, int& kind) {
    if (auto f = olxmed::check_grid(*g)) return grid_fail(c, who, f);
    double hmin = 1e300;
    for (int a = 0; a < 3; ++a) hmin = std::min(hmin, g->spacing[a]);
    const double to_rad = (apod_kind & OLX_APOD_RADIANS) ? 1.0 : (3.14159265358979323846 / 180.0);
    kind = apod_kind & ~OLX_APOD_RADIANS;
    if (kind < 0 || kind > 2) return fail(c, OLX_EINVAL, "%s: unknown apod_kind %d", who, apod_kind);
    if (!std::isfinite(p0) || (kind != OLX_APOD_UNIFORM && !(p0 >= 0))) return fail(c, OLX_EINVAL, "%s: apodization parameter must be finite (angles >= 0)", who);
    if (kind == OLX_APOD_PIECEWISE && !(p1 < p0 && p1 >= 0)) return fail(c, OLX_EINVAL, "%s: rolloff must be >= 0 and < zero angle", who);
    P.n_el = c->n_el;
    P.nx = g->n[0]; P.ny = g->n[1]; P.nz = g->n[2];
    P.vox = (long long)P.nx * P.ny * P.nz;
    P.ox = g->origin[0]; P.oy = g->origin[1]; P.oz = g->origin[2];
    P.hx = g->spacing[0]; P.hy = g->spacing[1]; P.hz = g->spacing[2];
    P.dmin2 = (float)(0.25 * hmin * hmin);
    P.value = kind == OLX_APOD_UNIFORM ? (float)p0 : 1.0f;
    P.lim2 = 2.0;      // every angle passes
    if (kind != OLX_APOD_UNIFORM) {
        const double lim = p0 * to_rad, half_pi = 1.5707963267948966;
        if (kind == OLX_APOD_MAXANGLE ? lim < half_pi : lim <= half_pi) { const double s = std::sin(lim); P.lim2 = s * s; }
        if (kind == OLX_APOD_PIECEWISE) { const double span = (p0 - p1) * to_rad; P.pw_scale = (float)(1.0 / span); P.pw_off = (float)(lim / span); }
    }
    return OLX_OK;
}

int olx_steer_map(olx_ctx* c, const olx_grid* g, double freq, double cs, double p0_pa, int apod_kind, double p0, double p1,
                  double absorption_np_m, unsigned flags, float* pfocal_out, int* n_active_out) {
    if (!c) return OLX_EINVAL;
    if (!g || !pfocal_out) return fail(c, OLX_EINVAL, "olx_steer_map: null grid or output");
    if (c->n_el <= 0) return fail(c, OLX_ESTATE, "olx_steer_map: call olx_set_elements first");
    if (flags & ~(unsigned)OLX_FIELD_DIRECTIVITY) return fail(c, OLX_EINVAL, "olx_steer_map: flags must be 0 or OLX_FIELD_DIRECTIVITY");
    const bool dir = (flags & OLX_FIELD_DIRECTIVITY) != 0;
    if (dir && c->h_xaxis.empty()) return fail(c, OLX_ESTATE, "olx_steer_map: OLX_FIELD_DIRECTIVITY needs olx_set_element_apertures");
    if (!(freq > 0) || !(cs > 0) || !std::isfinite(freq) || !std::isfinite(cs) || !std::isfinite(p0_pa))
        return fail(c, OLX_EINVAL, "olx_steer_map: freq and c must be finite and > 0, p0_pa finite");
    if (!(absorption_np_m >= 0) || !std::isfinite(absorption_np_m)) return fail(c, OLX_EINVAL, "olx_steer_map: absorption must be finite and >= 0");
    SteerParams P{}; int kind;
    { int rc = steer_params(c, "olx_steer_map", g, apod_kind, p0, p1, P, kind); if (rc) return rc; }
    if ((long long)P.nx * P.ny * ((P.nz + 3) / 4) > (long long)INT_MAX * 128) return fail(c, OLX_EINVAL, "olx_steer_map: grid too large");
    P.absorb_l2 = (float)(absorption_np_m * 1.4426950408889634);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)c->n_el;
    int rc = c->d_sm_p.reserve(c, (size_t)P.vox);
    if (!rc) rc = c->d_sm_n.reserve(c, (size_t)P.vox);
    if (!rc) rc = c->d_sm_tabd.reserve(c, n * STEER_TD);
    if (!rc) rc = c->d_sm_tabf.reserve(c, n * STEER_TF);
    if (!rc && dir) rc = c->d_sm_ap.reserve(c, n * 5);
    if (rc) return rc;
    if (dir) {
        HIPCHK(c, hipMemcpyAsync(c->d_sm_ap, c->h_xaxis.data(), sizeof(double) * 3 * n, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync((double*)c->d_sm_ap + 3 * n, c->h_size.data(), sizeof(double) * 2 * n, hipMemcpyHostToDevice, c->stream));
    }
    olx_launch_steer_table(c, dir ? (const double*)c->d_sm_ap : nullptr, p0_pa * freq / cs, 0.5 * freq / cs);
    HIPCHK(c, hipGetLastError());
    olx_launch_steer_map(c, P, kind, dir);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));     // (a large fetch runs on streams of its own, not ordered after this one)
    c->sm = P; c->sm_kind = kind; c->sm_dir = dir; c->sm_valid = true; c->sm_medium = false;
    rc = fetch_to_host(c, pfocal_out, c->d_sm_p, sizeof(float) * (size_t)P.vox);
    if (!rc && n_active_out) rc = fetch_to_host(c, n_active_out, c->d_sm_n, sizeof(int) * (size_t)P.vox);
    return rc;
}

// ---- kernel 4h: steering map through a heterogeneous medium (DESIGN.md section 2 "Steering map through a medium") ----
// Kernel 4's element records and decisions, kernel 2h's stencil and plane bounds; every buffer it writes is its own (d_smm_*) or kernel 4's element
// records: the plan and its medium, the steering table, the media of kernels 1m / 1a and every resident result stay as they are.
int olx_steer_map_medium(olx_ctx* c, const olx_grid* g, double freq, double cs, double p0_pa, int apod_kind, double p0, double p1,
                         const float* sound_speed, const float* attenuation, int comp, int spreading, int delays, unsigned flags,
                         float* pfocal_out, int* n_active_out) {
    if (!c) return OLX_EINVAL;
    if (!g || !pfocal_out) return fail(c, OLX_EINVAL, "olx_steer_map_medium: null grid or output");
    if (c->n_el <= 0) return fail(c, OLX_ESTATE, "olx_steer_map_medium: call olx_set_elements first");
    if (flags & ~(unsigned)OLX_FIELD_DIRECTIVITY) return fail(c, OLX_EINVAL, "olx_steer_map_medium: flags must be 0 or OLX_FIELD_DIRECTIVITY");
    const bool dir = (flags & OLX_FIELD_DIRECTIVITY) != 0;
    if (dir && c->h_xaxis.empty()) return fail(c, OLX_ESTATE, "olx_steer_map_medium: OLX_FIELD_DIRECTIVITY needs olx_set_element_apertures");
    if (!(freq > 0) || !(cs > 0) || !std::isfinite(freq) || !std::isfinite(cs) || !std::isfinite(p0_pa))
        return fail(c, OLX_EINVAL, "olx_steer_map_medium: freq and c_ref must be finite and > 0, p0_pa finite");
    if (comp != OLX_STEER_COMP_NONE && comp != OLX_COMP_EQUALIZE && comp != OLX_COMP_MATCHED)
        return fail(c, OLX_EINVAL, "olx_steer_map_medium: unknown comp %d", comp);
    if (delays != OLX_STEER_DELAYS_STRAIGHTRAY && delays != OLX_STEER_DELAYS_DIRECT)
        return fail(c, OLX_EINVAL, "olx_steer_map_medium: unknown delays %d", delays);
    SteerMedParams M{};
    SteerParams& P = M.S; int kind;
    { int rc = steer_params(c, "olx_steer_map_medium", g, apod_kind, p0, p1, P, kind); if (rc) return rc; }
    const int nx = g->n[0], ny = g->n[1], nz = g->n[2];
    const size_t nvox = (size_t)nx * ny * nz;
    // (32-bit byte offsets into a stencil plane of 32 bytes per cell, 24-bit factors; one block per 8 x 8 x 16 voxels)
    if ((long long)nx * ny > (1ll << 26) || nx >= (1 << 24) || ny >= (1 << 24) ||
        (long long)((nx + 7) / 8) * ((ny + 7) / 8) * ((nz + 15) / 16) > (long long)INT_MAX)
        return fail(c, OLX_EINVAL, "olx_steer_map_medium: grid too large");
    if (olxmed::first_bad(sound_speed, nvox, olxmed::POSITIVE) < nvox) return fail(c, OLX_EINVAL, "olx_steer_map_medium: sound speed must be finite and > 0");
    if (olxmed::first_bad(attenuation, nvox, olxmed::NON_NEGATIVE) < nvox) return fail(c, OLX_EINVAL, "olx_steer_map_medium: attenuation must be finite and >= 0");
    const bool phase = delays == OLX_STEER_DELAYS_DIRECT;
    const float* ssv = phase ? sound_speed : nullptr;      // StraightRay delays put every term in phase: the sound speed does not enter
    const double lambda = cs / freq;
    M.inv_hx = 1.0 / P.hx; M.inv_hy = 1.0 / P.hy;
    M.hz_w = (float)(P.hz / lambda);
    M.abs_value = std::fabs(P.value);
    M.spreading = spreading ? 1 : 0;
    // non-trivial planes and their pre-gathered stencil (kernel 2h's layout and conversions, power 0.9 as kernel 1a)
    const double afac = olxmed::np_per_m_factor(freq, 0.9) * lambda;      // dB/cm/MHz^0.9 -> Np per wavelength
    const auto [plane_of_k, plane_k] = olxmed::scan_planes(ssv, cs, attenuation, nx, ny, nz);
    const int np = M.n_planes = (int)plane_k.size();
    const std::vector<float> med = olxmed::gather_stencil(olxmed::plane_cells(ssv, cs, attenuation, afac, (size_t)nx * ny, nz, plane_k), np, nx, ny);
    // per element: first plane strictly above, last plane strictly below (olxmed::element_plane_bounds: kernel 2h's table entries), and S_e
    const size_t n = (size_t)c->n_el;
    const auto [kfirst, klast] = olxmed::element_plane_bounds(c->h_pos.data() + 2 * n, c->n_el, P.oz, P.hz, nz);
    std::vector<float> tabm(n * STEER_TM);
    for (size_t e = 0; e < n; ++e) {
        float* t = &tabm[e * STEER_TM];
        memcpy(&t[0], &kfirst[e], 4); memcpy(&t[1], &klast[e], 4);
        t[2] = (float)c->h_area[e]; t[3] = (float)(1.0 / c->h_area[e]);
    }
    HIPCHK(c, hipSetDevice(c->device));
    int rc = c->d_smm_p.reserve(c, nvox);
    if (!rc) rc = c->d_smm_n.reserve(c, nvox);
    if (!rc) rc = c->d_sm_tabd.reserve(c, n * STEER_TD);
    if (!rc) rc = c->d_sm_tabf.reserve(c, n * STEER_TF);
    if (!rc) rc = c->d_smm_tabm.reserve(c, n * STEER_TM);
    if (!rc) rc = c->d_smm_med.reserve(c, med.size() / 4);
    if (!rc) rc = c->d_smm_plane_k.reserve(c, np);
    if (!rc) rc = c->d_smm_plane_of_k.reserve(c, nz);
    if (!rc && dir) rc = c->d_sm_ap.reserve(c, n * 5);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));      // (the pageable copies below must not overtake a map still running on the stream)
    HIPCHK(c, hipMemcpy(c->d_smm_med, med.data(), sizeof(float) * med.size(), hipMemcpyHostToDevice));
    if (np) HIPCHK(c, hipMemcpy(c->d_smm_plane_k, plane_k.data(), sizeof(int) * np, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_smm_plane_of_k, plane_of_k.data(), sizeof(int) * nz, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_smm_tabm, tabm.data(), sizeof(float) * tabm.size(), hipMemcpyHostToDevice));
    if (dir) {
        HIPCHK(c, hipMemcpy(c->d_sm_ap, c->h_xaxis.data(), sizeof(double) * 3 * n, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy((double*)c->d_sm_ap + 3 * n, c->h_size.data(), sizeof(double) * 2 * n, hipMemcpyHostToDevice));
    }
    olx_launch_steer_table(c, dir ? (const double*)c->d_sm_ap : nullptr, p0_pa * freq / cs, 0.5 * freq / cs);
    HIPCHK(c, hipGetLastError());
    const int kcomp = comp == OLX_STEER_COMP_NONE ? 0 : (comp == OLX_COMP_EQUALIZE ? 1 : 2);
    olx_launch_steer_map_medium(c, M, kind, kcomp, phase, dir);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));     // (a large fetch runs on streams of its own, not ordered after this one)
    c->smm = M; c->sm_kind = kind; c->sm_dir = dir; c->smm_comp = kcomp; c->smm_phase = phase; c->sm_valid = true; c->sm_medium = true;
    rc = fetch_to_host(c, pfocal_out, c->d_smm_p, sizeof(float) * nvox);
    if (!rc && n_active_out) rc = fetch_to_host(c, n_active_out, c->d_smm_n, sizeof(int) * nvox);
    return rc;
}

int olx_steer_time(olx_ctx* c, int iters, float* ms_each) {
    if (!c) return OLX_EINVAL;
    if (iters < 1 || !ms_each) return fail(c, OLX_EINVAL, "olx_steer_time: iters < 1 or null output");
    if (!c->sm_valid) return fail(c, OLX_ESTATE, "olx_steer_time: no olx_steer_map to repeat");
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<hipEvent_t> ev(iters + 1, nullptr);
    for (auto& e : ev) HIPCHK(c, hipEventCreate(&e));
    HIPCHK(c, hipEventRecord(ev[0], c->stream));
    for (int i = 0; i < iters; ++i) {   // the element records are still those of the last map: olx_set_elements clears sm_valid
        if (c->sm_medium) olx_launch_steer_map_medium(c, c->smm, c->sm_kind, c->smm_comp, c->smm_phase, c->sm_dir);
        else olx_launch_steer_map(c, c->sm, c->sm_kind, c->sm_dir);
        HIPCHK(c, hipEventRecord(ev[i + 1], c->stream));
    }
    hipError_t e = hipStreamSynchronize(c->stream);
    for (int i = 0; i < iters && e == hipSuccess; ++i) e = hipEventElapsedTime(&ms_each[i], ev[i], ev[i + 1]);
    for (auto& v : ev) hipEventDestroy(v);
    if (e != hipSuccess) return fail(c, OLX_EHIP, "olx_steer_time: %s", hipGetErrorString(e));
    return OLX_OK;
}

int olx_field(olx_ctx* c, const olx_grid* g, int n_foci, double freq, double cs, double rho, double p0_pa,
              float* pmag_out, float* intensity_out) {
    if (!c) return OLX_EINVAL;
    unsigned flags = OLX_OUT_PMAG | (intensity_out ? OLX_OUT_INTENSITY : 0u);
    int rc = olx_field_plan(c, g, nullptr, n_foci, freq, cs, rho, p0_pa, flags);
    if (rc) return rc;
    rc = olx_field_launch(c);
    if (rc) return rc;
    const size_t vox = (size_t)c->fp.vox;
    for (int f = 0; f < n_foci; ++f) {
        rc = olx_field_fetch(c, f, pmag_out ? pmag_out + vox * f : nullptr,
                             intensity_out ? intensity_out + vox * f : nullptr, nullptr);
        if (rc) return rc;
    }
    return OLX_OK;
}

int olx_field_set_medium(olx_ctx* c, const float* sound_speed, const float* attenuation, const float* density,
                         double alpha_power) {
    if (!c) return OLX_EINVAL;
    if (!c->planned || c->uploaded) return fail(c, OLX_ESTATE, "olx_field_set_medium: call olx_field_plan first");
    if (c->directivity) return fail(c, OLX_EINVAL, "olx_field_set_medium: OLX_FIELD_DIRECTIVITY is not available with a heterogeneous medium");
    if (c->pulsed) return fail(c, OLX_EINVAL, "olx_field_set_medium: the pulsed model (olx_field_pulse) has no heterogeneous-medium kernel");
    if (c->plan_absorb > 0) return fail(c, OLX_EINVAL, "olx_field_set_medium: a uniform absorption (olx_field_absorption) and a heterogeneous medium exclude each other: put the absorption into the medium volumes");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const olx_grid& g = c->grid;
    const int nx = g.n[0], ny = g.n[1], nz = g.n[2], n = c->n_el;
    const size_t nvox = (size_t)nx * ny * nz;
    const double c0 = c->c, lambda = c->c / c->freq, rev = c->freq / c->c;
    const double afac = olxmed::np_per_wavelength_factor(c->freq, alpha_power, lambda);
    const auto [plane_of_k, plane_k] = olxmed::scan_planes(sound_speed, c0, attenuation, nx, ny, nz);      // the non-trivial planes
    const int np = (int)plane_k.size();
    // (known difference: +inf passes here, the other four entry points ask for finite values; unifying it would change behaviour)
    if (olxmed::first_bad(sound_speed, nvox, olxmed::POSITIVE, false) < nvox) return fail(c, OLX_EINVAL, "olx_field_set_medium: sound speed must be > 0");
    const std::vector<float> med = olxmed::gather_stencil(olxmed::plane_cells(sound_speed, c0, attenuation, afac, (size_t)nx * ny, nz, plane_k), np, nx, ny);
    // per element: first plane strictly above, last plane strictly below (fp64, same predicate as the oracle)
    const auto [kfirst, klast] = olxmed::element_plane_bounds(c->h_pos.data() + 2 * (size_t)n, n, g.origin[2], g.spacing[2], nz);
    // marched ray sums (kernel 2m) need rays that cross the non-trivial planes upwards only, and a 2 x 2 stencil
    bool march_ok = c->planes_per_layer == 1 && nx >= 2 && ny >= 2 && (size_t)n * nx * ny * sizeof(float2) < ((size_t)1 << 32);   // (32-bit lane offsets into U)
    if (np > 0)
        for (int e = 0; e < n && march_ok; ++e)
            if (!(c->h_pos[2 * (size_t)n + e] < g.origin[2] + plane_k[0] * g.spacing[2])) march_ok = false;
    if (c->medium_model == OLX_MEDIUM_MARCHED && !march_ok)
        return fail(c, OLX_EINVAL, "olx_field_set_medium: OLX_MEDIUM_MARCHED needs every element strictly below the first non-trivial "
                                    "plane, >= 2 voxels along x and y and planes_per_layer = 1");
    c->marched = march_ok && c->medium_model != OLX_MEDIUM_SAMPLED;
    // kernel 2m's one-sum form (olxmed::detect_one_line): a two-material medium over a lossless reference, water + skull
    c->march_one = false; c->hp.kappa = 0.f;
    if (c->marched && np > 0) {
        const olxmed::OneLine L = olxmed::detect_one_line(med, (size_t)np * nx * ny);
        const char* pin = getenv("OLX_MARCH_SUMS");
        if (L.one && L.s_ref != 0.0 && !(pin && !strcmp(pin, "2"))) { c->march_one = true; c->hp.kappa = (float)(L.a_ref / L.s_ref); }
    }
    if (c->march_one) {     // row-pair form of the last running sums (k_hmarch.hip TEX): 8 bytes per cell + one cell of padding, 32-bit byte offsets like U
        { int rc = c->d_Utex.reserve(c, (size_t)n * nx * ny + 1); if (rc) return rc; }
    }
    c->h_plane_k = plane_k;
    // the medium buffers belong to this medium: freed here, allocated again below only where this medium needs them (a null d_inv2z,
    // d_med_layer or d_sig means something to the kernels)
    c->d_med.release(); c->d_plane_k.release(); c->d_plane_of_k.release(); c->d_inv2z.release(); c->d_kfirst.release(); c->d_klast.release();
    c->d_med_layer.release(); c->d_layer_lo.release(); c->d_layer_hi.release(); c->d_sig.release();
    if (c->march_one && np > 0) {   // compact copy of the planes' own slowness terms for the fused writers (k_hmarch.hip, field_hmarch_fused_k)
        std::vector<float> sig((size_t)np * nx * ny);
        for (size_t q = 0; q < sig.size(); ++q) sig[q] = med[q * 8];
        { int rc = c->d_sig.reserve(c, sig.size()); if (rc) return rc; }
        HIPCHK(c, hipMemcpy(c->d_sig, sig.data(), sizeof(float) * sig.size(), hipMemcpyHostToDevice));
    }
    if (c->marched)
        for (DevBuf<float2>& u : c->d_U) { int rc = u.reserve(c, (size_t)n * nx * ny); if (rc) return rc; }
    // two-level quadrature (opt-in, olx_field_medium_layering): olxmed::layer_runs, a layer's stencil holds the column sums of its planes
    std::vector<int> layer_lo, layer_hi;
    if (c->planes_per_layer > 1) {
        olxmed::layer_runs(plane_k, c->planes_per_layer, layer_lo, layer_hi);
        const int nl = (int)layer_lo.size();
        const std::vector<float> lay = olxmed::gather_stencil(olxmed::layer_cells(sound_speed, c0, attenuation, afac, (size_t)nx * ny, nz, layer_lo, layer_hi), nl, nx, ny);
        int rc = c->d_med_layer.reserve(c, lay.size() / 4);
        if (!rc) rc = c->d_layer_lo.reserve(c, nl);
        if (!rc) rc = c->d_layer_hi.reserve(c, nl);
        if (rc) return rc;
        HIPCHK(c, hipMemcpy(c->d_med_layer, lay.data(), sizeof(float) * lay.size(), hipMemcpyHostToDevice));
        if (nl) {
            HIPCHK(c, hipMemcpy(c->d_layer_lo, layer_lo.data(), sizeof(int) * nl, hipMemcpyHostToDevice));
            HIPCHK(c, hipMemcpy(c->d_layer_hi, layer_hi.data(), sizeof(int) * nl, hipMemcpyHostToDevice));
        }
    }
    {
        int rc = c->d_med.reserve(c, med.size() / 4);
        if (!rc) rc = c->d_plane_k.reserve(c, np);
        if (!rc) rc = c->d_plane_of_k.reserve(c, nz);
        if (!rc) rc = c->d_kfirst.reserve(c, n);
        if (!rc) rc = c->d_klast.reserve(c, n);
        if (rc) return rc;
    }
    HIPCHK(c, hipMemcpy(c->d_med, med.data(), sizeof(float) * med.size(), hipMemcpyHostToDevice));
    if (np) HIPCHK(c, hipMemcpy(c->d_plane_k, plane_k.data(), sizeof(int) * np, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_plane_of_k, plane_of_k.data(), sizeof(int) * nz, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_kfirst, kfirst.data(), sizeof(int) * n, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_klast, klast.data(), sizeof(int) * n, hipMemcpyHostToDevice));
    if (density || sound_speed) {  // per-voxel 1e-4 / (2 rho c) for the intensity (sim/kwave_if.py:140-141), slab part
        const size_t sv = (size_t)c->fp.vox, off = (size_t)c->slab.x_begin * ny * nz;
        const std::vector<float> iz = olxmed::impedance_volume(density, c->rho, sound_speed, c0, off, sv);
        { int rc = c->d_inv2z.reserve(c, sv); if (rc) return rc; }
        HIPCHK(c, hipMemcpy(c->d_inv2z, iz.data(), sizeof(float) * sv, hipMemcpyHostToDevice));
    }
    if (c->derive_i) {      // kernels 2h / 2m store their intensity (it may carry a per-voxel impedance): back to the stored form
        c->derive_i = false; c->inten_live = false;
        { int rc = c->d_inten.reserve(c, c->d_pmag[0].capacity()); if (rc) return rc; }
        c->fp.flags |= OLX_OUT_INTENSITY; c->sp.flags |= OLX_OUT_INTENSITY;
    }
    HeteroParams& H = c->hp;
    H.n_planes = np; H.n_layers = (int)layer_lo.size(); H.n_foci = c->plan_foci; H.nxg = nx; H.nyg = ny; H.xg_begin = c->slab.x_begin;
    H.inv_hx = (float)(1.0 / (g.spacing[0] * rev)); H.inv_hy = (float)(1.0 / (g.spacing[1] * rev));
    H.u0 = 0.f; H.v0 = 0.f;  // table origin == grid origin for kernel 2h
    c->hetero = true;
    c->plan_ppl = c->planes_per_layer;      // (the layering this medium was built with: what the variant names, whatever olx_field_medium_layering says later)
    c->packed_version = ~0ull;
    return configure_variant(c);
}

int olx_field_absorption(olx_ctx* c, double np_per_m) {
    if (!c) return OLX_EINVAL;
    if (!(np_per_m >= 0) || !std::isfinite(np_per_m)) return fail(c, OLX_EINVAL, "olx_field_absorption: absorption must be finite and >= 0");
    c->absorb_np_m = np_per_m;
    return OLX_OK;
}

int olx_field_pulse(olx_ctx* c, double cycles, double dt, int n_t) {
    if (!c) return OLX_EINVAL;
    if (n_t < 0) return fail(c, OLX_EINVAL, "olx_field_pulse: n_t must be >= 0 (0 = continuous wave)");
    if (n_t > 0 && (!(cycles > 0) || !std::isfinite(cycles) || !(dt > 0) || !std::isfinite(dt)))
        return fail(c, OLX_EINVAL, "olx_field_pulse: cycles and dt must be finite and > 0");
    c->pulse_nt = n_t;
    c->pulse_cycles = n_t > 0 ? cycles : 0.0;
    c->pulse_dt = n_t > 0 ? dt : 0.0;
    return OLX_OK;
}

// Drive impulse responses of the pulsed model for the plans that follow: checked and kept on the host; olx_field_plan forms gamma from them
// with its own f0 dt (plan_pulse).  Nothing here touches the device.
int olx_field_pulse_response(olx_ctx* c, int n_classes, const int32_t* class_of_element, const int32_t* row, const double* taps) {
    if (!c) return OLX_EINVAL;
    if (n_classes == 0) { c->resp_cls.clear(); c->resp_row.clear(); c->resp_taps.clear(); return OLX_OK; }
    if (c->n_el <= 0) return fail(c, OLX_ESTATE, "olx_field_pulse_response: call olx_set_elements first");
    if (n_classes < 0 || n_classes > OLX_PULSE_RESPONSE_MAX_CLASSES)
        return fail(c, OLX_EINVAL, "olx_field_pulse_response: %d classes, at most OLX_PULSE_RESPONSE_MAX_CLASSES = %d (0 clears the response)", n_classes,
                    OLX_PULSE_RESPONSE_MAX_CLASSES);
    if (!class_of_element || !row || !taps) return fail(c, OLX_EINVAL, "olx_field_pulse_response: null pointer");
    if (row[0] != 0) return fail(c, OLX_EINVAL, "olx_field_pulse_response: the row table must start at 0, got %d", (int)row[0]);
    for (int r = 0; r < n_classes; ++r) {
        if (row[r + 1] <= row[r]) return fail(c, OLX_EINVAL, "olx_field_pulse_response: the row table must be strictly increasing (class %d has no taps)", r);
        if (row[r + 1] - row[r] > OLX_PULSE_RESPONSE_MAX_TAPS)
            return fail(c, OLX_EINVAL, "olx_field_pulse_response: class %d has %d taps, at most OLX_PULSE_RESPONSE_MAX_TAPS = %d", r, (int)(row[r + 1] - row[r]),
                        OLX_PULSE_RESPONSE_MAX_TAPS);
    }
    for (int e = 0; e < c->n_el; ++e)
        if (class_of_element[e] < 0 || class_of_element[e] >= n_classes)
            return fail(c, OLX_EINVAL, "olx_field_pulse_response: element %d: class %d outside 0 .. %d", e, (int)class_of_element[e], n_classes - 1);
    for (int g = 0; g < row[n_classes]; ++g)
        if (!std::isfinite(taps[g])) return fail(c, OLX_EINVAL, "olx_field_pulse_response: tap %d is not finite", g);
    c->resp_cls.assign(class_of_element, class_of_element + c->n_el);
    c->resp_row.assign(row, row + n_classes + 1);
    c->resp_taps.assign(taps, taps + row[n_classes]);
    return OLX_OK;
}

// Kernel 2ph: the medium of the CURRENT pulsed plan (DESIGN.md section 2 "Pulsed model through a medium").  Buffers and a flag of its own
// (pulse_med, d_pm_*): `hetero` selects the CW machinery -- the 2h / 2m launch, the d_inv2z readers -- and stays false.  A pulsed plan stores
// its intensity, so every scan reads this result as it reads kernel 2p's.
int olx_field_pulse_medium(olx_ctx* c, const float* sound_speed, const float* attenuation, const float* density, double alpha_power) {
    if (!c) return OLX_EINVAL;
    if (!c->planned || c->uploaded || !c->pulsed)
        return fail(c, OLX_ESTATE, "olx_field_pulse_medium: needs a pulsed plan (olx_field_pulse, then olx_field_plan)");
    if (c->presp_classes > 0)
        return fail(c, OLX_EINVAL, "olx_field_pulse_medium: the plan carries a drive impulse response (olx_field_pulse_response); kernel 2ph has none");
    if (c->plan_absorb > 0 || c->absorb_np_m > 0)
        return fail(c, OLX_EINVAL, "olx_field_pulse_medium: a uniform absorption (olx_field_absorption) and a heterogeneous medium exclude each other: put the absorption into the medium volumes");
    if (c->n_el != c->pulse.n_el) return fail(c, OLX_ESTATE, "olx_field_pulse_medium: the element table changed since the plan");
    if (c->n_el > 1024)
        return fail(c, OLX_EINVAL, "olx_field_pulse_medium: %d elements, kernel 2ph caches the ray sums of at most 1024 (16 per lane)", c->n_el);
    if (!std::isfinite(alpha_power)) return fail(c, OLX_EINVAL, "olx_field_pulse_medium: alpha_power must be finite");
    const olx_grid& g = c->grid;
    const int nx = g.n[0], ny = g.n[1], nz = g.n[2], n = c->n_el;
    const size_t nvox = (size_t)nx * ny * nz;
    // the three volumes voxel by voxel: the lowest bad index wins, ties go sound speed, attenuation, density
    const size_t bad[3] = {olxmed::first_bad(sound_speed, nvox, olxmed::POSITIVE), olxmed::first_bad(attenuation, nvox, olxmed::NON_NEGATIVE), olxmed::first_bad(density, nvox, olxmed::POSITIVE)};
    switch (olxmed::first_bad_volume(bad, 3, nvox)) {
        case 0: return fail(c, OLX_EINVAL, "olx_field_pulse_medium: sound speed must be finite and > 0");
        case 1: return fail(c, OLX_EINVAL, "olx_field_pulse_medium: attenuation must be finite and >= 0");
        case 2: return fail(c, OLX_EINVAL, "olx_field_pulse_medium: density must be finite and > 0");
    }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const double c0 = c->c;
    const double afac = olxmed::np_per_m_factor(c->freq, alpha_power);
    const auto [plane_of_k, plane_k] = olxmed::scan_planes(sound_speed, c0, attenuation, nx, ny, nz);      // the non-trivial planes
    const int np = (int)plane_k.size();
    const size_t nxy = (size_t)nx * ny;
    // compact [plane][i][j] arrays: sig = c_ref / c - 1 in fp64 from the float32 volume, a in Np/m rounded once; one zero where no plane is held
    std::vector<double> sig; std::vector<float> att;
    if (sound_speed) { sig = olxmed::plane_sigma(sound_speed, c0, nxy, nz, plane_k); sig.resize(std::max<size_t>(sig.size(), 1)); }
    if (attenuation) { att = olxmed::plane_att(attenuation, afac, nxy, nz, plane_k); att.resize(std::max<size_t>(att.size(), 1)); }
    const auto [kfirst, klast] = olxmed::element_plane_bounds(c->h_pos.data() + 2 * (size_t)n, n, g.origin[2], g.spacing[2], nz);
    std::vector<int2> kb(n);      // per element: first plane strictly above, last plane strictly below
    for (int e = 0; e < n; ++e) kb[e] = make_int2(kfirst[e], klast[e]);
    c->pulse_med = false;      // (until everything below is in place)
    int rc = c->d_pm_plane_k.reserve(c, np);
    if (!rc) rc = c->d_pm_plane_of_k.reserve(c, nz);
    if (!rc) rc = c->d_pm_kb.reserve(c, n);
    if (!rc && sound_speed) rc = c->d_pm_sig.reserve(c, sig.size());
    if (!rc && attenuation) rc = c->d_pm_att.reserve(c, att.size());
    if (rc) return rc;
    if (np) HIPCHK(c, hipMemcpy(c->d_pm_plane_k, plane_k.data(), sizeof(int) * np, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_pm_plane_of_k, plane_of_k.data(), sizeof(int) * nz, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_pm_kb, kb.data(), sizeof(int2) * n, hipMemcpyHostToDevice));
    if (sound_speed) HIPCHK(c, hipMemcpy(c->d_pm_sig, sig.data(), sizeof(double) * sig.size(), hipMemcpyHostToDevice));
    if (attenuation) HIPCHK(c, hipMemcpy(c->d_pm_att, att.data(), sizeof(float) * att.size(), hipMemcpyHostToDevice));
    c->pm_has_sig = sound_speed != nullptr; c->pm_has_att = attenuation != nullptr; c->pm_has_z = density || sound_speed;
    if (c->pm_has_z) {      // per-voxel 1e-4 / (2 rho c) of the intensity and the PII (sim/kwave_if.py:140-141)
        const std::vector<float> iz = olxmed::impedance_volume(density, c->rho, sound_speed, c0, 0, nvox);
        rc = c->d_pm_inv2z.reserve(c, nvox);
        if (rc) return rc;
        HIPCHK(c, hipMemcpy(c->d_pm_inv2z, iz.data(), sizeof(float) * nvox, hipMemcpyHostToDevice));
    }
    PulseMedParams& M = c->pm;
    M.P = c->pulse;
    M.nx = nx; M.n_planes = np;
    M.inv_hx = 1.0 / g.spacing[0]; M.inv_hy = 1.0 / g.spacing[1];
    M.two_dt = (float)(2.0 * c->pulse_plan_dt);
    c->pulse_med_R = n <= 256 ? 4 : 16;
    c->pulse_med = true;      // (resident volumes of an earlier launch of this plan stay what that launch made them)
    char nm[160];
    snprintf(nm, sizeof nm, "field_pulse_med_k (pulsed through a medium: %d samples, %d planes, R = %d)", c->pulse.n_t, np, c->pulse_med_R);
    c->variant = nm;
    return OLX_OK;
}

int olx_field_medium_layering(olx_ctx* c, int planes_per_layer) {
    if (!c) return OLX_EINVAL;
    if (planes_per_layer < 1 || planes_per_layer > 4096) return fail(c, OLX_EINVAL, "olx_field_medium_layering: planes_per_layer must be in [1, 4096]");
    c->planes_per_layer = planes_per_layer;
    return OLX_OK;
}

int olx_field_medium_model(olx_ctx* c, int model) {
    if (!c) return OLX_EINVAL;
    if (model != OLX_MEDIUM_AUTO && model != OLX_MEDIUM_SAMPLED && model != OLX_MEDIUM_MARCHED)
        return fail(c, OLX_EINVAL, "olx_field_medium_model: unknown model %d", model);
    c->medium_model = model;
    return OLX_OK;
}

int olx_field_upload(olx_ctx* c, const olx_grid* g, const olx_slab* slab, int n_foci, const float* pmag,
                     const float* intensity) {
    if (!c) return OLX_EINVAL;
    if (!g || !pmag || n_foci < 1) return fail(c, OLX_EINVAL, "olx_field_upload: null grid / volume or n_foci < 1");
    for (int a = 0; a < 3; ++a)
        if (g->n[a] < 1 || !(g->spacing[a] > 0)) return fail(c, OLX_EINVAL, "olx_field_upload: bad grid axis %d", a);
    olx_slab s{0, g->n[0]};
    if (slab) s = *slab;
    if (s.x_begin < 0 || s.x_count < 1 || s.x_begin + s.x_count > g->n[0]) return fail(c, OLX_EINVAL, "olx_field_upload: slab outside grid");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const long long vox = (long long)s.x_count * g->n[1] * g->n[2];
    pii_regrid(c, vox);
    const size_t total = (size_t)vox * n_foci;
    { int rc_ = exported_buffers_quiesce(c, -1); if (rc_) return rc_; }   // (p2p: buffer 0 is rewritten, all of them may be freed)
    c->derive_i = false; c->inten_live = false;      // (an uploaded intensity is whatever the caller says it is)
    { int rc_ = reserve_outputs(c, total, 1, intensity != nullptr, false, false); if (rc_) return rc_; }
    HIPCHK(c, hipMemcpy(c->d_pmag[0], pmag, sizeof(float) * total, hipMemcpyHostToDevice));
    if (intensity) HIPCHK(c, hipMemcpy(c->d_inten, intensity, sizeof(float) * total, hipMemcpyHostToDevice));
    c->grid = *g; c->slab = s; c->plan_foci = n_foci;
    c->agg_local = -1; c->agg_total = 0;   // like olx_field_plan: the counts of a former padded sweep do not describe these volumes
    c->hetero = false; c->marched = false; c->pulse_med = false;
    c->pulsed = false; c->pmax_live = false; c->agg_pmax_valid = false; c->pii_live = false;    // (an upload holds no p_max and no PII)
    c->fp.nx = s.x_count; c->fp.ny = g->n[1]; c->fp.nz = g->n[2]; c->fp.vox = vox;
    c->flags = OLX_OUT_PMAG | (intensity ? OLX_OUT_INTENSITY : 0u);
    c->cur = 0; c->nbuf = 1;
    c->planned = true; c->uploaded = true;
    c->variant = "uploaded";
    return OLX_OK;
}

int olx_field_time(olx_ctx* c, int iters, float* ms_each) {
    if (!c) return OLX_EINVAL;
    if (iters < 1 || !ms_each) return fail(c, OLX_EINVAL, "olx_field_time: iters < 1 or null output");
    if (!c->planned) return fail(c, OLX_ESTATE, "olx_field_time: nothing planned");
    HIPCHK(c, hipSetDevice(c->device));
    struct Events {
        std::vector<hipEvent_t> ev;
        ~Events() { for (auto e : ev) if (e) hipEventDestroy(e); }
    } T;
    T.ev.assign(iters + 1, nullptr);
    std::vector<hipEvent_t>& ev = T.ev;
    for (auto& e : ev) HIPCHK(c, hipEventCreate(&e));
    int rc = c->pulsed ? OLX_OK : pack_if_needed(c);     // (kernel 2p builds its own table at every launch)
    if (rc) return rc;
    HIPCHK(c, hipEventRecord(ev[0], c->stream));
    for (int i = 0; i < iters; ++i) {
        rc = olx_field_launch(c);
        if (rc) break;
        HIPCHK(c, hipEventRecord(ev[i + 1], c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (!rc)
        for (int i = 0; i < iters; ++i) HIPCHK(c, hipEventElapsedTime(&ms_each[i], ev[i], ev[i + 1]));
    return rc;
}

static int aggregate_local(olx_ctx* c, bool with_p, bool with_i);
// Pulsed plans: what the scans do to |p| (the p_min slot) they do to the resident p_max volumes as well -- scale them by the per-focus
// factors already on the device (`scale`: F floats, NULL = no scaling) and, with `aggregate`, form max_f p_max_f.  Nothing without them.
static int pmax_post(olx_ctx* c, const float* scale, bool aggregate) {
    if (!c->pmax_live) return OLX_OK;
    if (scale) hipLaunchKernelGGL(field_scale_k, dim3(1024, c->plan_foci), dim3(256), 0, c->stream, c->d_pmax, (float*)nullptr, (float*)nullptr, scale, c->fp.vox);
    if (aggregate) {
        { int rc = c->d_agg_pmax.reserve(c, (size_t)c->fp.vox); if (rc) return rc; }
        hipLaunchKernelGGL(field_aggregate_k<false>, dim3(2048), dim3(256), 0, c->stream, c->d_pmax, (const float*)nullptr, c->plan_foci, (long long)c->fp.vox,
                           1.0f / (float)c->plan_foci, 0.f, c->d_agg_pmax, (float*)nullptr);
    }
    HIPCHK(c, hipGetLastError());
    if (aggregate) c->agg_pmax_valid = true;
    return OLX_OK;
}
}
static void fill_scan_params(const olx_ctx* c, PeakParams& P, const double* aspect);
static int pii_scan_time(olx_ctx* c, int kernel, int iters, float* ms_each, double* bytes_per_launch);
// Blocks per focus of the masked scans: ~2048 blocks in flight over all foci (8 per CU, all resident), each living long enough
// that its one-thread mask preparation (fp32 frame, band, first plane above zmin) does not count -- with 2048 blocks PER focus a
// block moved 32 KB and the prologue was most of its life.
static unsigned scan_blocks(long long want, int F) {
    const long long per_focus = std::max<long long>(2048 / std::max(F, 1), 128);
    return (unsigned)std::max<long long>(1, std::min(want, per_focus));
}
// the fused post-pass for the planned row length and intensity mode
static auto saa_kernel(const olx_ctx* c) -> decltype(&field_scale_agg_analyze_k<false, false>) {
    const bool rowq = (c->fp.nz & 3) != 0;
    if (c->derive_i) return rowq ? field_scale_agg_analyze_k<true, true> : field_scale_agg_analyze_k<false, true>;
    return rowq ? field_scale_agg_analyze_k<true, false> : field_scale_agg_analyze_k<false, false>;
}

extern "C" {

// Streaming scans over the resident result, timed like olx_field_time: `iters` back-to-back launches of ONE scan kernel on the
// context's stream, a HIP event between each.  These are the HBM-bound kernels of the path; *bytes_per_launch
// receives the algorithmic traffic of one launch so that the caller can quote GB/s against the roofline.
int olx_scan_time(olx_ctx* c, int kernel, int iters, float* ms_each, double* bytes_per_launch) {
    if (!c) return OLX_EINVAL;
    if (iters < 1 || !ms_each || !bytes_per_launch) return fail(c, OLX_EINVAL, "olx_scan_time: iters < 1 or null output");
    if (!c->planned) return fail(c, OLX_ESTATE, "olx_scan_time: nothing planned");
    if (kernel == OLX_SCAN_PII_SCALE || kernel == OLX_SCAN_PII_FULL) return pii_scan_time(c, kernel, iters, ms_each, bytes_per_launch);
    if (kernel < 0 || kernel > OLX_SCAN_FUSED_POST) return fail(c, OLX_EINVAL, "olx_scan_time: unknown kernel %d", kernel);
    if (kernel == OLX_SCAN_FUSED_POST && (c->plan_foci > SAA_MAXF || (long long)c->fp.nx * c->fp.ny * ((c->fp.nz + 3) / 4) >= (1ll << 31))) return fail(c, OLX_ESTATE, "olx_scan_time: the fused pass needs <= 8 foci and < 2^31 row quads");
    if (!(c->flags & OLX_OUT_INTENSITY)) return fail(c, OLX_ESTATE, "olx_scan_time: intensity not planned");
    HIPCHK(c, hipSetDevice(c->device));
    if (kernel == OLX_SCAN_SCALE || kernel == OLX_SCAN_FUSED_POST) { int rc_ = exported_buffers_quiesce(c, c->cur); if (rc_) return rc_; }
    if (kernel == OLX_SCAN_AGGREGATE || kernel == OLX_SCAN_FUSED_POST) { int rc_ = aggregate_buffers_free(c); if (rc_) return rc_; }
    const int F = c->plan_foci;
    const double vox = (double)c->fp.vox;
    struct Events {
        std::vector<hipEvent_t> ev;
        ~Events() { for (auto e : ev) if (e) hipEventDestroy(e); }
    } T;
    T.ev.assign(iters + 1, nullptr);
    for (auto& e : T.ev) HIPCHK(c, hipEventCreate(&e));
    // a focal frame per focus: axes = grid axes, origin = the grid centre (a mainlobe-sized mask in the middle of the volume)
    DevScratch scratch;
    const size_t n_ax = (size_t)c->fp.nx + c->fp.ny + c->fp.nz;
    const size_t og_bytes = kernel == OLX_SCAN_OFFSET_GRID ? sizeof(double) * 4 * (size_t)c->fp.vox : 0;
    HIPCHK(c, hipMalloc(&scratch.p, sizeof(double) * (12 * (size_t)F + n_ax) + sizeof(unsigned) * 6 * F + sizeof(float) * F + og_bytes + 64));
    double* d_A = scratch.at<double>(0);
    double* d_ax = d_A + 12 * (size_t)F;
    unsigned* d_pk = reinterpret_cast<unsigned*>(d_ax + n_ax);
    float* d_w = reinterpret_cast<float*>(d_pk + 6 * (size_t)F);
    double* d_og = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(d_w + F) + 63) & ~(uintptr_t)63);
    {
        std::vector<double> hA(12 * (size_t)F, 0.0), hax(n_ax);
        const double ctr[3] = {c->grid.origin[0] + (c->slab.x_begin + 0.5 * (c->fp.nx - 1)) * c->grid.spacing[0],
                               c->grid.origin[1] + 0.5 * (c->fp.ny - 1) * c->grid.spacing[1], c->grid.origin[2] + 0.5 * (c->fp.nz - 1) * c->grid.spacing[2]};
        for (int f = 0; f < F; ++f) for (int a = 0; a < 3; ++a) { hA[12 * (size_t)f + 4 * a + a] = 1.0; hA[12 * (size_t)f + 4 * a + 3] = -ctr[a]; }
        size_t k = 0;
        for (int i = 0; i < c->fp.nx; ++i) hax[k++] = c->grid.origin[0] + (c->slab.x_begin + i) * c->grid.spacing[0];
        for (int i = 0; i < c->fp.ny; ++i) hax[k++] = c->grid.origin[1] + i * c->grid.spacing[1];
        for (int i = 0; i < c->fp.nz; ++i) hax[k++] = c->grid.origin[2] + i * c->grid.spacing[2];
        std::vector<float> hw(F, 1.0f / (float)F);
        HIPCHK(c, hipMemcpy(d_A, hA.data(), sizeof(double) * hA.size(), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(d_ax, hax.data(), sizeof(double) * hax.size(), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(d_w, hw.data(), sizeof(float) * F, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemset(d_pk, 0, sizeof(unsigned) * 6 * F));
    }
    if (kernel == OLX_SCAN_WEIGHTED_SUM || kernel == OLX_SCAN_FUSED_POST) { int rc_ = c->d_wint.reserve(c, (size_t)c->fp.vox); if (rc_) return rc_; }
    if (kernel == OLX_SCAN_FUSED_POST) {
        { int rc_ = aggregate_buffers_free(c); if (rc_) return rc_; }
        { int rc_ = reserve_aggregate(c, true, true); if (rc_) return rc_; }
    }
    if (kernel == OLX_SCAN_SCALE || kernel == OLX_SCAN_FUSED_POST) {
        { int rc_ = c->d_scale.reserve(c, 4096); if (rc_) return rc_; }
        if (F > 4096) return fail(c, OLX_EINVAL, "olx_scan_time: too many foci");
        std::vector<float> one(F, 1.0f);        // x 1.0f is exact: the resident result is unchanged
        HIPCHK(c, hipMemcpy(c->d_scale, one.data(), sizeof(float) * F, hipMemcpyHostToDevice));
    }
    const double asp[3] = {1.0, 1.0, 5.0};
    PeakParams P; fill_scan_params(c, P, asp);
    P.radius = 2.5e-3; P.op = 0; P.use_zmin = 1; P.zmin = c->grid.origin[2] + c->grid.spacing[2];
    const long long want = (P.vox + 255) / 256;
    const bool D = c->derive_i; const float IK_ = c->fp.inten_scale;
    HIPCHK(c, hipEventRecord(T.ev[0], c->stream));
    for (int i = 0; i < iters; ++i) {
        switch (kernel) {
        // (bytes: what the launched form moves -- a deriving plan reads and writes |p| only, half the per-focus traffic of the stored form)
        case OLX_SCAN_AGGREGATE: { int rc = aggregate_local(c, true, true); if (rc) return rc; *bytes_per_launch = vox * ((D ? 4.0 : 8.0) * F + 8.0); break; }
        case OLX_SCAN_SCALE:
            hipLaunchKernelGGL(field_scale_k, dim3(1024, F), dim3(256), 0, c->stream, c->d_pmag[c->cur], inten_arg(c), (float*)nullptr, c->d_scale, c->fp.vox);
            *bytes_per_launch = vox * (D ? 8.0 : 16.0) * F; break;
        case OLX_SCAN_ANALYSIS_PEAKS:      // (the form olx_solution_analyze launches)
            if ((c->fp.nz & 3) == 0 && c->fp.vox < (1ll << 33))
                hipLaunchKernelGGL(D ? field_analysis_peaks4_k<true> : field_analysis_peaks4_k<false>, dim3(scan_blocks(want, F), F), dim3(256), 0, c->stream, c->d_pmag[c->cur], inten_arg(c), d_A, P, 5e-3, IK_, d_pk);
            else
                hipLaunchKernelGGL(D ? field_analysis_peaks_k<true> : field_analysis_peaks_k<false>, dim3((unsigned)std::min<long long>(want, 2048), F), dim3(256), 0, c->stream, c->d_pmag[c->cur], inten_arg(c), d_A, P, 5e-3, IK_, d_pk);
            *bytes_per_launch = vox * (D ? 4.0 : 8.0) * F; break;
        case OLX_SCAN_MASKED_PEAK:         // an OUTSIDE mask ('>': every voxel is visited; inside masks only visit their index box)
            P.op = 2;
            hipLaunchKernelGGL(field_masked_peak_k, dim3(scan_blocks(want, F), F), dim3(256), 0, c->stream, c->d_pmag[c->cur], d_A, P, d_pk);
            *bytes_per_launch = vox * 4.0 * F; break;
        case OLX_SCAN_OFFSET_GRID:
            hipLaunchKernelGGL(offset_grid_k, dim3((unsigned)std::min<long long>(want, 4096)), dim3(256), 0, c->stream, d_ax, d_ax + c->fp.nx, d_ax + c->fp.nx + c->fp.ny,
                               c->fp.nx, c->fp.ny, c->fp.nz, d_A, 1.0, 1.0, 0.2, d_og, d_og + 3 * (size_t)c->fp.vox);
            *bytes_per_launch = vox * 32.0; break;
        case OLX_SCAN_FUSED_POST:          // scale (by 1.0) + aggregate + six peaks + time-average volume in one pass
            P.op = 0;
            hipLaunchKernelGGL(saa_kernel(c), dim3(2048), dim3(256), 0, c->stream, c->d_pmag[c->cur], inten_arg(c), c->d_scale, d_w, d_A, F, P, 5e-3,
                               1.0f / (float)F, IK_, c->d_agg_p, c->d_agg_i, c->d_wint, d_pk, d_pk + 6 * (size_t)F - 1);
            *bytes_per_launch = vox * ((D ? 8.0 : 16.0) * F + 12.0); break;
        default:
            hipLaunchKernelGGL(D ? field_weighted_sum_k<true> : field_weighted_sum_k<false>, dim3(2048), dim3(256), 0, c->stream, D ? c->d_pmag[c->cur] : c->d_inten, d_w, F, c->fp.vox, IK_, c->d_wint);
            *bytes_per_launch = vox * (4.0 * F + 4.0); break;
        }
        HIPCHK(c, hipEventRecord(T.ev[i + 1], c->stream));
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < iters; ++i) HIPCHK(c, hipEventElapsedTime(&ms_each[i], T.ev[i], T.ev[i + 1]));
    return OLX_OK;
}

const char* olx_field_variant(const olx_ctx* c) { return (c && c->planned) ? c->variant.c_str() : ""; }

// max |p| / mean intensity over the planned foci into the aggregate buffers (device only)
static int aggregate_local(olx_ctx* c, bool with_p, bool with_i) {
    const size_t vox = (size_t)c->fp.vox;
    { int rc_ = aggregate_buffers_free(c); if (rc_) return rc_; }
    if (with_p) { int rc_ = pmax_post(c, nullptr, true); if (rc_) return rc_; }
    { int rc_ = reserve_aggregate(c, with_p, with_i); if (rc_) return rc_; }
    if (c->derive_i)     // (the mean of the intensities the |p| volumes define: |p| is read whether or not its maximum is wanted)
        hipLaunchKernelGGL(field_aggregate_k<true>, dim3(2048), dim3(256), 0, c->stream, c->d_pmag[c->cur], nullptr, c->plan_foci, (long long)vox,
                           1.0f / (float)c->plan_foci, c->fp.inten_scale, with_p ? c->d_agg_p : nullptr, with_i ? c->d_agg_i : nullptr);
    else
    hipLaunchKernelGGL(field_aggregate_k<false>, dim3(2048), dim3(256), 0, c->stream, with_p ? c->d_pmag[c->cur] : nullptr,
                       with_i ? c->d_inten : nullptr, c->plan_foci, (long long)vox, 1.0f / (float)c->plan_foci, 0.f,
                       with_p ? c->d_agg_p : nullptr, with_i ? c->d_agg_i : nullptr);
    HIPCHK(c, hipGetLastError());
    return OLX_OK;
}

int olx_field_aggregate(olx_ctx* c, float* pmax_out, float* imean_out) {
    if (!c) return OLX_EINVAL;
    if (!c->planned) return fail(c, OLX_ESTATE, "olx_field_aggregate: nothing planned");
    if (imean_out && !(c->flags & OLX_OUT_INTENSITY)) return fail(c, OLX_ESTATE, "olx_field_aggregate: intensity not planned");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t vox = (size_t)c->fp.vox;
    int rc = aggregate_local(c, pmax_out != nullptr, imean_out != nullptr);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // the two aggregate volumes go to pageable caller memory through the pipelined staged copy of the per-focus fetches
    // (a plain hipMemcpy to pageable memory moves ~12 GB/s here, the staged copy 25 - 45)
    if (pmax_out) rc = fetch_to_host(c, pmax_out, c->d_agg_p, sizeof(float) * vox);
    if (!rc && imean_out) rc = fetch_to_host(c, imean_out, c->d_agg_i, sizeof(float) * vox);
    return rc;
}

int olx_field_aggregate_device(olx_ctx* c, int want_intensity) {
    if (!c) return OLX_EINVAL;
    if (!c->planned) return fail(c, OLX_ESTATE, "olx_field_aggregate_device: nothing planned");
    if (want_intensity && !(c->flags & OLX_OUT_INTENSITY)) return fail(c, OLX_ESTATE, "olx_field_aggregate_device: intensity not planned");
    HIPCHK(c, hipSetDevice(c->device));
    return aggregate_local(c, true, want_intensity != 0);
}

int olx_field_scale(olx_ctx* c, const double* scale, int n_foci) {
    if (!c) return OLX_EINVAL;
    if (!c->planned) return fail(c, OLX_ESTATE, "olx_field_scale: nothing planned");
    if (!scale || n_foci != c->plan_foci) return fail(c, OLX_EINVAL, "olx_field_scale: need %d scale factors", c->plan_foci);
    HIPCHK(c, hipSetDevice(c->device));
    { int rc_ = c->d_scale.reserve(c, 4096); if (rc_) return rc_; }
    if (n_foci > 4096) return fail(c, OLX_EINVAL, "olx_field_scale: too many foci");
    { int rc_ = exported_buffers_quiesce(c, c->cur); if (rc_) return rc_; }   // (p2p: no peer may pull a half-scaled block)
    std::vector<float> s(n_foci);
    for (int i = 0; i < n_foci; ++i) s[i] = (float)scale[i];
    HIPCHK(c, hipMemcpyAsync(c->d_scale, s.data(), sizeof(float) * n_foci, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(field_scale_k, dim3(1024, n_foci), dim3(256), 0, c->stream, c->d_pmag[c->cur],
                       (c->flags & OLX_OUT_INTENSITY) ? inten_arg(c) : nullptr,      // (a deriving plan scales |p| only: intensity x s^2 follows from olx_inten)
                       (c->flags & OLX_OUT_COMPLEX) ? c->d_cplx : nullptr, c->d_scale, c->fp.vox);
    c->inten_live = false;
    HIPCHK(c, hipGetLastError());
    { int rc_ = pmax_post(c, c->d_scale, false); if (rc_) return rc_; }
    c->agg_pmax_valid = false;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return OLX_OK;
}

// olx_field_scale + olx_field_aggregate_device in one pass over the volumes (what Protocol.calc_solution(scale=True) does back to
// back): identical values, a third less HBM traffic.  Falls back to the two separate kernels when the fused form does not apply
// (complex output planned, voxel count not a multiple of 4).
int olx_field_scale_aggregate(olx_ctx* c, const double* scale, int n_foci) {
    if (!c) return OLX_EINVAL;
    if (!c->planned) return fail(c, OLX_ESTATE, "olx_field_scale_aggregate: nothing planned");
    if (!scale || n_foci != c->plan_foci) return fail(c, OLX_EINVAL, "olx_field_scale_aggregate: need %d scale factors", c->plan_foci);
    if (!(c->flags & OLX_OUT_INTENSITY)) return fail(c, OLX_ESTATE, "olx_field_scale_aggregate: intensity not planned");
    if (n_foci > 4096) return fail(c, OLX_EINVAL, "olx_field_scale_aggregate: too many foci");
    if ((c->flags & OLX_OUT_COMPLEX) || (c->fp.vox & 3)) {
        int rc = olx_field_scale(c, scale, n_foci);
        return rc ? rc : olx_field_aggregate_device(c, 1);
    }
    HIPCHK(c, hipSetDevice(c->device));
    { int rc_ = c->d_scale.reserve(c, 4096); if (rc_) return rc_; }
    { int rc_ = exported_buffers_quiesce(c, c->cur); if (rc_) return rc_; }   // (p2p: the volumes are scaled in place)
    { int rc_ = aggregate_buffers_free(c); if (rc_) return rc_; }
    { int rc_ = reserve_aggregate(c, true, true); if (rc_) return rc_; }
    std::vector<float> s(n_foci);
    for (int i = 0; i < n_foci; ++i) s[i] = (float)scale[i];
    HIPCHK(c, hipMemcpyAsync(c->d_scale, s.data(), sizeof(float) * n_foci, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(c->derive_i ? field_scale_aggregate_k<true> : field_scale_aggregate_k<false>, dim3(4096), dim3(256), 0, c->stream, c->d_pmag[c->cur], inten_arg(c), c->d_scale, n_foci,
                       (long long)c->fp.vox, 1.0f / (float)n_foci, c->fp.inten_scale, c->d_agg_p, c->d_agg_i);
    c->inten_live = false;
    HIPCHK(c, hipGetLastError());
    { int rc_ = pmax_post(c, c->d_scale, true); if (rc_) return rc_; }
    HIPCHK(c, hipStreamSynchronize(c->stream));      // (s lives on this frame)
    return OLX_OK;
}

// Index box [x0, x1) x [y0, y1) x [z0, z1) (slab indices) that encloses the focal ellipsoid |diag(1 / aspect) . A_f . [r, 1]| <= radius
// of every focus, with one voxel of margin: half-extent along axis i = radius * sqrt((M^-1)_ii), M = B^T B, B = diag(1 / aspect) . A_3x3.
// A degenerate frame (singular B) gets the whole slab.
static void focus_boxes(const olx_ctx* c, const double* A, const double* aspect, double radius, int F, int* boxes) {
    const int n[3] = {c->fp.nx, c->fp.ny, c->fp.nz};
    const double o[3] = {c->grid.origin[0] + c->slab.x_begin * c->grid.spacing[0], c->grid.origin[1], c->grid.origin[2]};
    for (int f = 0; f < F; ++f) {
        const double* a = A + 12 * (size_t)f;
        double B[3][3], t[3];
        for (int r = 0; r < 3; ++r) { for (int k = 0; k < 3; ++k) B[r][k] = a[4 * r + k] / aspect[r]; t[r] = a[4 * r + 3] / aspect[r]; }
        double M[3][3];
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) M[i][j] = B[0][i] * B[0][j] + B[1][i] * B[1][j] + B[2][i] * B[2][j];
        const double det = M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
                           M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
        int* b = boxes + 6 * (size_t)f;
        if (!(std::fabs(det) > 1e-300) || !(radius >= 0)) { for (int i = 0; i < 3; ++i) { b[2 * i] = 0; b[2 * i + 1] = n[i]; } continue; }
        const double inv_diag[3] = {(M[1][1] * M[2][2] - M[1][2] * M[2][1]) / det, (M[0][0] * M[2][2] - M[0][2] * M[2][0]) / det,
                                    (M[0][0] * M[1][1] - M[0][1] * M[1][0]) / det};
        // centre: B c + t = 0  ->  c = -M^-1 B^T t (solved through the adjugate of M)
        const double bt[3] = {B[0][0] * t[0] + B[1][0] * t[1] + B[2][0] * t[2], B[0][1] * t[0] + B[1][1] * t[1] + B[2][1] * t[2],
                              B[0][2] * t[0] + B[1][2] * t[1] + B[2][2] * t[2]};
        const double adj[3][3] = {{M[1][1] * M[2][2] - M[1][2] * M[2][1], M[0][2] * M[2][1] - M[0][1] * M[2][2], M[0][1] * M[1][2] - M[0][2] * M[1][1]},
                                  {M[1][2] * M[2][0] - M[1][0] * M[2][2], M[0][0] * M[2][2] - M[0][2] * M[2][0], M[0][2] * M[1][0] - M[0][0] * M[1][2]},
                                  {M[1][0] * M[2][1] - M[1][1] * M[2][0], M[0][1] * M[2][0] - M[0][0] * M[2][1], M[0][0] * M[1][1] - M[0][1] * M[1][0]}};
        for (int i = 0; i < 3; ++i) {
            const double ctr = -(adj[i][0] * bt[0] + adj[i][1] * bt[1] + adj[i][2] * bt[2]) / det;
            const double half = radius * std::sqrt(std::max(inv_diag[i], 0.0)) * (1.0 + 1e-9);
            const double h = i == 0 ? c->grid.spacing[0] : c->grid.spacing[i];
            const double lo = std::floor((ctr - half - o[i]) / h) - 1.0, hi = std::ceil((ctr + half - o[i]) / h) + 2.0;
            b[2 * i] = (int)std::min(std::max(lo, 0.0), (double)n[i]);
            b[2 * i + 1] = (int)std::min(std::max(hi, 0.0), (double)n[i]);
        }
    }
}

static int analysis_scratch(olx_ctx* c, size_t dev_bytes, size_t host_bytes) {
    { int rc = c->d_an.reserve(c, dev_bytes); if (rc) return rc; }
    if (c->h_an_bytes < host_bytes) {
        if (c->h_an) hipHostFree(c->h_an);
        c->h_an = nullptr; c->h_an_bytes = 0;
        HIPCHK(c, hipHostMalloc(&c->h_an, host_bytes, hipHostMallocDefault));
        c->h_an_bytes = host_bytes;
    }
    return OLX_OK;
}

int olx_field_masked_peak(olx_ctx* c, int which, const double* A, const double* aspect, double radius_m, int op,
                          int use_zmin, double zmin_m, float* peak_out) {
    if (!c) return OLX_EINVAL;
    if (!c->planned) return fail(c, OLX_ESTATE, "olx_field_masked_peak: nothing planned");
    if (!peak_out || !aspect || op < 0 || op > 4 || (op != 4 && !A)) return fail(c, OLX_EINVAL, "olx_field_masked_peak: bad arguments");
    if (which == 1 && !(c->flags & OLX_OUT_INTENSITY)) return fail(c, OLX_ESTATE, "olx_field_masked_peak: intensity not planned");
    if (which < 0 || which > 2) return fail(c, OLX_EINVAL, "olx_field_masked_peak: which must be 0, 1 or 2");
    if (which == 2 && !c->d_wint) return fail(c, OLX_ESTATE, "olx_field_masked_peak: call olx_field_weighted_intensity first");
    HIPCHK(c, hipSetDevice(c->device));
    const int F = c->plan_foci;
    {
        int rc = c->d_peakA.reserve(c, 12 * (size_t)F);
        if (!rc) rc = c->d_peak.reserve(c, F);
        if (rc) return rc;
    }
    if (A) HIPCHK(c, hipMemcpyAsync(c->d_peakA, A, sizeof(double) * 12 * F, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_peak, 0, sizeof(unsigned) * F, c->stream));
    PeakParams P;
    P.nx = c->fp.nx; P.ny = c->fp.ny; P.nz = c->fp.nz;
    P.ox = c->grid.origin[0] + c->slab.x_begin * c->grid.spacing[0]; P.oy = c->grid.origin[1]; P.oz = c->grid.origin[2];
    P.hx = c->grid.spacing[0]; P.hy = c->grid.spacing[1]; P.hz = c->grid.spacing[2];
    P.ia0 = 1.0 / aspect[0]; P.ia1 = 1.0 / aspect[1]; P.ia2 = 1.0 / aspect[2];
    P.radius = radius_m; P.op = op; P.use_zmin = use_zmin; P.zmin = zmin_m; P.vox = c->fp.vox;
    P.vol_stride = which == 2 ? 0 : c->fp.vox;
    const long long want = (P.vox + 255) / 256;
    dim3 grid(scan_blocks(want, F), F);
    if (which == 1) { int rc = materialize_intensity(c); if (rc) return rc; }
    const float* vol = which == 0 ? c->d_pmag[c->cur] : (which == 1 ? c->d_inten : c->d_wint);
    if (op <= 1) {   // inside-the-ellipsoid masks: only the index box around each focus' ellipsoid is visited (same per-voxel test)
        std::vector<int> boxes(6 * (size_t)F);
        focus_boxes(c, A, aspect, radius_m, F, boxes.data());
        { int rc = analysis_scratch(c, sizeof(int) * 6 * F, 0); if (rc) return rc; }
        HIPCHK(c, hipMemcpyAsync(c->d_an, boxes.data(), sizeof(int) * 6 * F, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(field_masked_peak_box_k, dim3(32, F), dim3(256), 0, c->stream, vol, c->d_peakA, P, reinterpret_cast<const int*>(static_cast<unsigned char*>(c->d_an)), c->d_peak);
        HIPCHK(c, hipStreamSynchronize(c->stream));   // (boxes lives on this frame)
    } else
    hipLaunchKernelGGL(field_masked_peak_k, grid, dim3(256), 0, c->stream, vol, c->d_peakA, P, c->d_peak);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(peak_out, c->d_peak, sizeof(float) * F, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return OLX_OK;
}

int olx_field_analysis_peaks(olx_ctx* c, const double* A, const double* aspect, double r_main_m, double r_side_m, double zmin_m,
                             float* peaks_out) {
    if (!c) return OLX_EINVAL;
    if (!c->planned) return fail(c, OLX_ESTATE, "olx_field_analysis_peaks: nothing planned");
    if (!A || !aspect || !peaks_out) return fail(c, OLX_EINVAL, "olx_field_analysis_peaks: null argument");
    if (!(c->flags & OLX_OUT_INTENSITY)) return fail(c, OLX_ESTATE, "olx_field_analysis_peaks: intensity not planned");
    HIPCHK(c, hipSetDevice(c->device));
    const int F = c->plan_foci;
    DevScratch scratch;   // [12 F] focal-frame rows (fp64) | [6 F] peaks
    HIPCHK(c, hipMalloc(&scratch.p, sizeof(double) * 12 * F + sizeof(unsigned) * 6 * F));
    double* d_A = scratch.at<double>(0);
    unsigned* d_out = scratch.at<unsigned>(sizeof(double) * 12 * F);
    HIPCHK(c, hipMemcpyAsync(d_A, A, sizeof(double) * 12 * F, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(d_out, 0, sizeof(unsigned) * 6 * F, c->stream));
    PeakParams P;
    P.nx = c->fp.nx; P.ny = c->fp.ny; P.nz = c->fp.nz;
    P.ox = c->grid.origin[0] + c->slab.x_begin * c->grid.spacing[0]; P.oy = c->grid.origin[1]; P.oz = c->grid.origin[2];
    P.hx = c->grid.spacing[0]; P.hy = c->grid.spacing[1]; P.hz = c->grid.spacing[2];
    P.ia0 = 1.0 / aspect[0]; P.ia1 = 1.0 / aspect[1]; P.ia2 = 1.0 / aspect[2];
    P.radius = r_main_m; P.op = 0; P.use_zmin = 1; P.zmin = zmin_m; P.vox = c->fp.vox; P.vol_stride = c->fp.vox;
    const long long want = (P.vox + 255) / 256;
    dim3 grid((unsigned)std::min<long long>(want, 2048), F);
    hipLaunchKernelGGL(c->derive_i ? field_analysis_peaks_k<true> : field_analysis_peaks_k<false>, grid, dim3(256), 0, c->stream, c->d_pmag[c->cur], inten_arg(c), d_A, P, r_side_m, c->fp.inten_scale, d_out);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(peaks_out, d_out, sizeof(float) * 6 * F, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return OLX_OK;
}

static void fill_scan_params(const olx_ctx* c, PeakParams& P, const double* aspect) {
    P.nx = c->fp.nx; P.ny = c->fp.ny; P.nz = c->fp.nz;
    P.ox = c->grid.origin[0] + c->slab.x_begin * c->grid.spacing[0]; P.oy = c->grid.origin[1]; P.oz = c->grid.origin[2];
    P.hx = c->grid.spacing[0]; P.hy = c->grid.spacing[1]; P.hz = c->grid.spacing[2];
    P.ia0 = aspect ? 1.0 / aspect[0] : 1.0; P.ia1 = aspect ? 1.0 / aspect[1] : 1.0; P.ia2 = aspect ? 1.0 / aspect[2] : 1.0;
    P.radius = 0; P.op = 0; P.use_zmin = 0; P.zmin = 0; P.vox = c->fp.vox; P.vol_stride = c->fp.vox;
}

// ---- pulse intensity integrals (pii_post_k) ---------------------------------------------------------------------------------------
}   // extern "C"
template <bool SCALE, bool WTS, bool PEAKS> static void launch_pii_post(olx_ctx* c, const PeakParams& P, double r_side, unsigned blocks, int F) {
    float* const gw = c->d_pii_gw;
    unsigned* const pk = c->d_pii_peak;
    if (P.nz & 3) hipLaunchKernelGGL((pii_post_k<SCALE, WTS, PEAKS, true>), dim3(blocks), dim3(256), 0, c->stream, (float*)c->d_pii, gw, gw + PII_MAXF,
                                     (const double*)c->d_pii_A, F, P, r_side, (float*)c->d_pii_w, (float*)c->d_pii_max, pk, pk + 4 * PII_MAXF);
    else hipLaunchKernelGGL((pii_post_k<SCALE, WTS, PEAKS, false>), dim3(blocks), dim3(256), 0, c->stream, (float*)c->d_pii, gw, gw + PII_MAXF,
                            (const double*)c->d_pii_A, F, P, r_side, (float*)c->d_pii_w, (float*)c->d_pii_max, pk, pk + 4 * PII_MAXF);
}
extern "C" {

int olx_pii_post(olx_ctx* c, const double* scale_per_focus, const double* weights, int n_foci, const double* A, const double* aspect,
                 double r_main_m, double r_side_m, double zmin_m, float* peaks_out) {
    if (!c) return OLX_EINVAL;
    if (!c->planned || !c->pii_live) return fail(c, OLX_ESTATE, "olx_pii_post: no resident pulse intensity integrals (a launched pulsed plan with OLX_OUT_PII, or olx_pii_upload)");
    if (n_foci != c->pii_foci) return fail(c, OLX_EINVAL, "olx_pii_post: %d foci given, the resident pulse intensity integrals have %d", n_foci, c->pii_foci);
    if (A && (!aspect || !peaks_out)) return fail(c, OLX_EINVAL, "olx_pii_post: focal frames need aspect and peaks_out");
    const int F = n_foci;
    if (F > PII_MAXF) return fail(c, OLX_EINVAL, "olx_pii_post: at most %d foci", PII_MAXF);
    const long long quads = (long long)c->fp.nx * c->fp.ny * ((c->fp.nz + 3) / 4);
    if (quads >= (1ll << 31)) return fail(c, OLX_EINVAL, "olx_pii_post: grid too large (2^31 row quads or more)");
    float gw[2 * PII_MAXF] = {0};
    for (int f = 0; f < F; ++f) {
        if (scale_per_focus && !std::isfinite(scale_per_focus[f])) return fail(c, OLX_EINVAL, "olx_pii_post: scale factor %d is not finite", f);
        if (weights && !(weights[f] >= 0 && std::isfinite(weights[f]))) return fail(c, OLX_EINVAL, "olx_pii_post: weight %d must be finite and >= 0", f);
        gw[f] = scale_per_focus ? (float)(scale_per_focus[f] * scale_per_focus[f]) : 1.f;
        gw[PII_MAXF + f] = weights ? (float)weights[f] : 0.f;
    }
    HIPCHK(c, hipSetDevice(c->device));
    {
        const size_t vox = (size_t)c->fp.vox;
        int rc = c->d_pii_gw.reserve(c, 2 * PII_MAXF);
        if (!rc) rc = c->d_pii_A.reserve(c, 12 * PII_MAXF);
        if (!rc) rc = c->d_pii_peak.reserve(c, 4 * PII_MAXF + 1);
        if (!rc) rc = c->d_pii_max.reserve(c, vox);
        if (!rc && weights) rc = c->d_pii_w.reserve(c, vox);
        if (rc) return rc;
    }
    if (scale_per_focus || weights) c->pii_w_valid = false;      // (scaled volumes leave an older weighted volume behind)
    c->pii_max_valid = false;
    HIPCHK(c, hipMemcpyAsync(c->d_pii_gw, gw, sizeof gw, hipMemcpyHostToDevice, c->stream));
    PeakParams P;
    fill_scan_params(c, P, aspect);
    if (A) {
        HIPCHK(c, hipMemcpyAsync(c->d_pii_A, A, sizeof(double) * 12 * F, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync(c->d_pii_peak, 0, sizeof(unsigned) * (4 * PII_MAXF + 1), c->stream));
        P.radius = r_main_m; P.use_zmin = 1; P.zmin = zmin_m;
    }
    const unsigned blocks = (unsigned)std::max<long long>(1, std::min<long long>((quads + 255) / 256, 2048));
    const int form = (scale_per_focus ? 4 : 0) | (weights ? 2 : 0) | (A ? 1 : 0);
    switch (form) {
        case 0: launch_pii_post<false, false, false>(c, P, r_side_m, blocks, F); break;
        case 1: launch_pii_post<false, false, true>(c, P, r_side_m, blocks, F); break;
        case 2: launch_pii_post<false, true, false>(c, P, r_side_m, blocks, F); break;
        case 3: launch_pii_post<false, true, true>(c, P, r_side_m, blocks, F); break;
        case 4: launch_pii_post<true, false, false>(c, P, r_side_m, blocks, F); break;
        case 5: launch_pii_post<true, false, true>(c, P, r_side_m, blocks, F); break;
        case 6: launch_pii_post<true, true, false>(c, P, r_side_m, blocks, F); break;
        default: launch_pii_post<true, true, true>(c, P, r_side_m, blocks, F); break;
    }
    HIPCHK(c, hipGetLastError());
    unsigned pk[4 * PII_MAXF + 1];
    if (A) HIPCHK(c, hipMemcpyAsync(pk, c->d_pii_peak, sizeof pk, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));      // (gw and pk live on this frame)
    if (A) {
        memcpy(peaks_out, pk, sizeof(float) * 4 * F);
        memcpy(peaks_out + 4 * F, pk + 4 * PII_MAXF, sizeof(float));
    }
    c->pii_max_valid = true;
    if (weights) c->pii_w_valid = true;
    return OLX_OK;
}

}   // extern "C"
// olx_scan_time of pii_post_k over the resident PII: the scale-only form (factors 1.0f: exact, the volumes stay as they are) or the full form
// (factors, weights 1 / F, a mainlobe-sized mask at the grid centre), `iters` launches back to back with a HIP event between each
static int pii_scan_time(olx_ctx* c, int kernel, int iters, float* ms_each, double* bytes_per_launch) {
    if (!c->pii_live) return fail(c, OLX_ESTATE, "olx_scan_time: no resident pulse intensity integrals");
    const int F = c->pii_foci;
    const long long quads = (long long)c->fp.nx * c->fp.ny * ((c->fp.nz + 3) / 4);
    if (F > PII_MAXF || quads >= (1ll << 31)) return fail(c, OLX_ESTATE, "olx_scan_time: pii_post_k needs <= %d foci and < 2^31 row quads", PII_MAXF);
    HIPCHK(c, hipSetDevice(c->device));
    const bool full = kernel == OLX_SCAN_PII_FULL;
    {
        const size_t vox = (size_t)c->fp.vox;
        int rc = c->d_pii_gw.reserve(c, 2 * PII_MAXF);
        if (!rc) rc = c->d_pii_A.reserve(c, 12 * PII_MAXF);
        if (!rc) rc = c->d_pii_peak.reserve(c, 4 * PII_MAXF + 1);
        if (!rc) rc = c->d_pii_max.reserve(c, vox);
        if (!rc && full) rc = c->d_pii_w.reserve(c, vox);
        if (rc) return rc;
    }
    c->pii_w_valid = false; c->pii_max_valid = false;
    float gw[2 * PII_MAXF];
    for (int f = 0; f < PII_MAXF; ++f) { gw[f] = 1.0f; gw[PII_MAXF + f] = 1.0f / (float)F; }
    double hA[12 * PII_MAXF] = {0};
    const double ctr[3] = {c->grid.origin[0] + (c->slab.x_begin + 0.5 * (c->fp.nx - 1)) * c->grid.spacing[0],
                           c->grid.origin[1] + 0.5 * (c->fp.ny - 1) * c->grid.spacing[1], c->grid.origin[2] + 0.5 * (c->fp.nz - 1) * c->grid.spacing[2]};
    for (int f = 0; f < F; ++f) for (int a = 0; a < 3; ++a) { hA[12 * f + 4 * a + a] = 1.0; hA[12 * f + 4 * a + 3] = -ctr[a]; }
    HIPCHK(c, hipMemcpy(c->d_pii_gw, gw, sizeof gw, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_pii_A, hA, sizeof hA, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemset(c->d_pii_peak, 0, sizeof(unsigned) * (4 * PII_MAXF + 1)));
    const double asp[3] = {1.0, 1.0, 5.0};
    PeakParams P; fill_scan_params(c, P, asp);
    P.radius = 2.5e-3; P.op = 0; P.use_zmin = 1; P.zmin = c->grid.origin[2] + c->grid.spacing[2];
    const unsigned blocks = (unsigned)std::max<long long>(1, std::min<long long>((quads + 255) / 256, 2048));
    struct Events {
        std::vector<hipEvent_t> ev;
        ~Events() { for (auto e : ev) if (e) hipEventDestroy(e); }
    } T;
    T.ev.assign(iters + 1, nullptr);
    for (auto& e : T.ev) HIPCHK(c, hipEventCreate(&e));
    HIPCHK(c, hipEventRecord(T.ev[0], c->stream));
    for (int i = 0; i < iters; ++i) {
        if (full) launch_pii_post<true, true, true>(c, P, 5e-3, blocks, F);
        else launch_pii_post<true, false, false>(c, P, 5e-3, blocks, F);
        HIPCHK(c, hipEventRecord(T.ev[i + 1], c->stream));
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < iters; ++i) HIPCHK(c, hipEventElapsedTime(&ms_each[i], T.ev[i], T.ev[i + 1]));
    *bytes_per_launch = (double)c->fp.vox * (8.0 * F + (full ? 8.0 : 4.0));
    c->pii_max_valid = true; c->pii_w_valid = full;
    return OLX_OK;
}
extern "C" {

int olx_pii_fetch_weighted(olx_ctx* c, float* out) {
    if (!c) return OLX_EINVAL;
    if (!out) return fail(c, OLX_EINVAL, "olx_pii_fetch_weighted: null output");
    if (!c->pii_live || !c->pii_w_valid) return fail(c, OLX_ESTATE, "olx_pii_fetch_weighted: no weighted volume of the resident pulse intensity integrals (olx_pii_post with weights)");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return fetch_to_host(c, out, c->d_pii_w, sizeof(float) * (size_t)c->fp.vox);
}

int olx_pii_fetch_max(olx_ctx* c, float* out) {
    if (!c) return OLX_EINVAL;
    if (!out) return fail(c, OLX_EINVAL, "olx_pii_fetch_max: null output");
    if (!c->pii_live || !c->pii_max_valid) return fail(c, OLX_ESTATE, "olx_pii_fetch_max: no maximum over foci of the resident pulse intensity integrals (olx_pii_post)");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return fetch_to_host(c, out, c->d_pii_max, sizeof(float) * (size_t)c->fp.vox);
}

int olx_pii_upload(olx_ctx* c, int n_foci, const float* pii) {
    if (!c) return OLX_EINVAL;
    if (!c->planned) return fail(c, OLX_ESTATE, "olx_pii_upload: no grid (olx_field_plan or olx_field_upload first)");
    if (!pii || n_foci < 1) return fail(c, OLX_EINVAL, "olx_pii_upload: null volume or n_foci < 1");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t total = (size_t)c->fp.vox * n_foci;
    c->pii_live = false; c->pii_w_valid = false; c->pii_max_valid = false;
    { int rc_ = c->d_pii.reserve(c, total); if (rc_) return rc_; }
    HIPCHK(c, hipMemcpy(c->d_pii, pii, sizeof(float) * total, hipMemcpyHostToDevice));
    c->pii_live = true; c->pii_foci = n_foci;
    return OLX_OK;
}

int olx_field_masked_moments(olx_ctx* c, const double* A, const double* aspect, double radius_m, const float* cutoff,
                             double* moments_out) {
    if (!c) return OLX_EINVAL;
    if (!c->planned) return fail(c, OLX_ESTATE, "olx_field_masked_moments: nothing planned");
    if (!A || !aspect || !cutoff || !moments_out) return fail(c, OLX_EINVAL, "olx_field_masked_moments: null argument");
    HIPCHK(c, hipSetDevice(c->device));
    const int F = c->plan_foci;
    DevScratch scratch;   // [12 F] focal-frame rows | [4 F] moments (fp64) | [F] cutoffs
    HIPCHK(c, hipMalloc(&scratch.p, sizeof(double) * 16 * F + sizeof(float) * F));
    double* d_A = scratch.at<double>(0);
    double* d_out = scratch.at<double>(sizeof(double) * 12 * F);
    float* d_cut = scratch.at<float>(sizeof(double) * 16 * F);
    HIPCHK(c, hipMemcpyAsync(d_A, A, sizeof(double) * 12 * F, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_cut, cutoff, sizeof(float) * F, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(d_out, 0, sizeof(double) * 4 * F, c->stream));
    PeakParams P; fill_scan_params(c, P, aspect); P.radius = radius_m;
    dim3 grid((unsigned)std::min<long long>((P.vox + 255) / 256, 1024), F);
    hipLaunchKernelGGL(field_masked_moments_k, grid, dim3(256), 0, c->stream, c->d_pmag[c->cur], d_A, d_cut, P, d_out);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(moments_out, d_out, sizeof(double) * 4 * F, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return OLX_OK;
}

int olx_field_sample(olx_ctx* c, int which, int focus, const double* pts_m, int npts, float* out) {
    if (!c) return OLX_EINVAL;
    if (!c->planned) return fail(c, OLX_ESTATE, "olx_field_sample: nothing planned");
    if (!pts_m || !out || npts < 1) return fail(c, OLX_EINVAL, "olx_field_sample: null argument or npts < 1");
    if (focus < 0 || focus >= c->plan_foci) return fail(c, OLX_EINVAL, "olx_field_sample: focus out of range");
    if (which != 0 && which != 1) return fail(c, OLX_EINVAL, "olx_field_sample: which must be 0 or 1");
    if (which == 1 && !(c->flags & OLX_OUT_INTENSITY)) return fail(c, OLX_ESTATE, "olx_field_sample: intensity not planned");
    HIPCHK(c, hipSetDevice(c->device));
    DevScratch scratch;   // [3 npts] points (fp64) | [npts] samples
    HIPCHK(c, hipMalloc(&scratch.p, sizeof(double) * 3 * npts + sizeof(float) * npts));
    double* d_pts = scratch.at<double>(0);
    float* d_o = scratch.at<float>(sizeof(double) * 3 * npts);
    HIPCHK(c, hipMemcpyAsync(d_pts, pts_m, sizeof(double) * 3 * npts, hipMemcpyHostToDevice, c->stream));
    PeakParams P; fill_scan_params(c, P, nullptr);
    if (which == 1) { int rc = materialize_intensity(c); if (rc) return rc; }
    const float* vol = (which == 0 ? c->d_pmag[c->cur] : c->d_inten) + (size_t)focus * c->fp.vox;
    hipLaunchKernelGGL(field_sample_k, dim3((npts + 127) / 128), dim3(128), 0, c->stream, vol, d_pts, npts, P, d_o);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, d_o, sizeof(float) * npts, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return OLX_OK;
}

int olx_offset_grid(olx_ctx* c, const double* xs, int nx, const double* ys, int ny, const double* zs, int nz, const double* A,
                    const double* aspect, double* coords_out, double* dist_out) {
    if (!c) return OLX_EINVAL;
    if (!xs || !ys || !zs || !A || nx < 1 || ny < 1 || nz < 1) return fail(c, OLX_EINVAL, "olx_offset_grid: null axis / matrix or empty grid");
    if (!coords_out && !dist_out) return fail(c, OLX_EINVAL, "olx_offset_grid: no output requested");
    if (dist_out && aspect) for (int a = 0; a < 3; ++a) if (!(aspect[a] != 0.0)) return fail(c, OLX_EINVAL, "olx_offset_grid: zero aspect ratio");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t vox = (size_t)nx * ny * nz;
    DevScratch ax, co, di;
    HIPCHK(c, hipMalloc(&ax.p, sizeof(double) * ((size_t)nx + ny + nz + 12)));
    if (coords_out && hipMalloc(&co.p, sizeof(double) * 3 * vox) != hipSuccess) return fail(c, OLX_ENOMEM, "olx_offset_grid: out of device memory");
    if (dist_out && hipMalloc(&di.p, sizeof(double) * vox) != hipSuccess) return fail(c, OLX_ENOMEM, "olx_offset_grid: out of device memory");
    double *d_ax = ax.at<double>(0), *d_c = co.at<double>(0), *d_d = di.at<double>(0);
    hipMemcpyAsync(d_ax, xs, sizeof(double) * nx, hipMemcpyHostToDevice, c->stream);
    hipMemcpyAsync(d_ax + nx, ys, sizeof(double) * ny, hipMemcpyHostToDevice, c->stream);
    hipMemcpyAsync(d_ax + nx + ny, zs, sizeof(double) * nz, hipMemcpyHostToDevice, c->stream);
    hipMemcpyAsync(d_ax + nx + ny + nz, A, sizeof(double) * 12, hipMemcpyHostToDevice, c->stream);
    const unsigned blocks = (unsigned)std::min<size_t>((vox + 255) / 256, 4096);
    hipLaunchKernelGGL(offset_grid_k, dim3(blocks), dim3(256), 0, c->stream, d_ax, d_ax + nx, d_ax + nx + ny, nx, ny, nz,
                       d_ax + nx + ny + nz, aspect ? 1.0 / aspect[0] : 1.0, aspect ? 1.0 / aspect[1] : 1.0, aspect ? 1.0 / aspect[2] : 1.0,
                       d_c, d_d);
    int rc = hipGetLastError() == hipSuccess ? OLX_OK : OLX_EHIP;
    if (!rc && coords_out && hipMemcpyAsync(coords_out, d_c, sizeof(double) * 3 * vox, hipMemcpyDeviceToHost, c->stream) != hipSuccess) rc = OLX_EHIP;
    if (!rc && dist_out && hipMemcpyAsync(dist_out, d_d, sizeof(double) * vox, hipMemcpyDeviceToHost, c->stream) != hipSuccess) rc = OLX_EHIP;
    if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) rc = OLX_EHIP;
    if (rc) return fail(c, OLX_EHIP, "olx_offset_grid: HIP error");
    return OLX_OK;
}

int olx_tof_spread(olx_ctx* c, const double* xs, int nx, const double* ys, int ny, const double* zs, int nz,
                   const double* delays_s, double c0, double* max_dtof_s) {
    if (!c) return OLX_EINVAL;
    if (c->n_el <= 0) return fail(c, OLX_ESTATE, "olx_tof_spread: call olx_set_elements first");
    if (!xs || !ys || !zs || !max_dtof_s || nx < 1 || ny < 1 || nz < 1 || !(c0 > 0)) return fail(c, OLX_EINVAL, "olx_tof_spread: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    const int n = c->n_el;
    DevScratch scratch;
    HIPCHK(c, hipMalloc(&scratch.p, sizeof(double) * ((size_t)nx + ny + nz + n + 1)));
    double* d_buf = scratch.at<double>(0);
    double* d_del = d_buf + nx + ny + nz;
    unsigned long long* d_out = reinterpret_cast<unsigned long long*>(d_del + n);
    hipMemcpyAsync(d_buf, xs, sizeof(double) * nx, hipMemcpyHostToDevice, c->stream);
    hipMemcpyAsync(d_buf + nx, ys, sizeof(double) * ny, hipMemcpyHostToDevice, c->stream);
    hipMemcpyAsync(d_buf + nx + ny, zs, sizeof(double) * nz, hipMemcpyHostToDevice, c->stream);
    if (delays_s) hipMemcpyAsync(d_del, delays_s, sizeof(double) * n, hipMemcpyHostToDevice, c->stream);
    hipMemsetAsync(d_out, 0, sizeof(unsigned long long), c->stream);
    const size_t vox = (size_t)nx * ny * nz;
    const unsigned blocks = (unsigned)std::min<size_t>((vox + 255) / 256, 8192);
    hipLaunchKernelGGL(tof_spread_k, dim3(blocks), dim3(256), 0, c->stream, d_buf, d_buf + nx, d_buf + nx + ny, nx, ny, nz, c->d_pos,
                       delays_s ? d_del : nullptr, n, c0, d_out);
    int rc = hipGetLastError() == hipSuccess ? OLX_OK : OLX_EHIP;
    unsigned long long bits = 0;
    if (!rc && hipMemcpyAsync(&bits, d_out, sizeof bits, hipMemcpyDeviceToHost, c->stream) != hipSuccess) rc = OLX_EHIP;
    if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) rc = OLX_EHIP;
    if (rc) return fail(c, OLX_EHIP, "olx_tof_spread: HIP error");
    memcpy(max_dtof_s, &bits, sizeof bits);
    return OLX_OK;
}

int olx_field_weighted_intensity(olx_ctx* c, const double* weights, int n_foci) {
    if (!c) return OLX_EINVAL;
    if (!c->planned) return fail(c, OLX_ESTATE, "olx_field_weighted_intensity: nothing planned");
    if (!(c->flags & OLX_OUT_INTENSITY)) return fail(c, OLX_ESTATE, "olx_field_weighted_intensity: intensity not planned");
    if (!weights || n_foci != c->plan_foci || n_foci > 4096) return fail(c, OLX_EINVAL, "olx_field_weighted_intensity: need %d weights", c->plan_foci);
    HIPCHK(c, hipSetDevice(c->device));
    {
        int rc = c->d_scale.reserve(c, 4096);
        if (!rc) rc = c->d_wint.reserve(c, (size_t)c->fp.vox);
        if (rc) return rc;
    }
    std::vector<float> w(n_foci);
    for (int i = 0; i < n_foci; ++i) w[i] = (float)weights[i];
    HIPCHK(c, hipMemcpyAsync(c->d_scale, w.data(), sizeof(float) * n_foci, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(c->derive_i ? field_weighted_sum_k<true> : field_weighted_sum_k<false>, dim3(2048), dim3(256), 0, c->stream, c->derive_i ? c->d_pmag[c->cur] : c->d_inten, c->d_scale, n_foci, c->fp.vox, c->fp.inten_scale, c->d_wint);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return OLX_OK;
}

int olx_field_weighted_fetch(olx_ctx* c, float* out) {
    if (!c || !out) return OLX_EINVAL;
    if (!c->planned || c->d_wint.capacity() < (size_t)c->fp.vox) return fail(c, OLX_ESTATE, "olx_field_weighted_fetch: no time-average volume on the device");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return fetch_to_host(c, out, c->d_wint, sizeof(float) * (size_t)c->fp.vox);
}

// ---- one-call analysis ------------------------------------------------------------------------------------------
// Solution.analyze used to cross the C-ABI ~40 times per 8-focus solution (6-peak scan, moments, weighted intensity, two masked
// peaks, 24 line samplings), every crossing with its own scratch hipMalloc / hipFree, pageable copies and a stream
// synchronisation: 7.6 of calc_solution's 11 ms.  Here the same kernels are enqueued back to back; the numbers that feed later
// steps (mainlobe peak -> -3 dB centroid cut-off, beam-width cut-offs) stay on the device; one pinned block goes in, one
// comes out, one synchronisation.  Scratch is owned by the context and reused.
int olx_solution_analyze_begin(olx_ctx* c, const double* A, const double* ita_weights, const double* line_pts,
                               const olx_analysis_opts* o, const double* scale_per_focus) {
    if (!c) return OLX_EINVAL;
    if (c->an_pending) {   // a begin without its finish: the earlier analysis' copies may still be reading / writing the pinned block this call rewrites
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->an_pending = false;
    }
    if (!c->planned) return fail(c, OLX_ESTATE, "olx_solution_analyze: nothing planned");
    if (!A || !ita_weights || !o) return fail(c, OLX_EINVAL, "olx_solution_analyze: null argument");
    if (!(c->flags & OLX_OUT_INTENSITY)) return fail(c, OLX_ESTATE, "olx_solution_analyze: intensity not planned");
    const int F = c->plan_foci;
    if (F > 4096) return fail(c, OLX_EINVAL, "olx_solution_analyze: too many foci");
    int npts = 0;
    BeamLines L{};
    for (int a = 0; a < 3; ++a) {
        if (o->n_line[a] < 0 || o->n_le[a] < 0 || o->n_le[a] > o->n_line[a] || o->i_ge[a] < 0 || o->i_ge[a] > o->n_line[a])
            return fail(c, OLX_EINVAL, "olx_solution_analyze: bad line description for axis %d", a);
        L.start[a] = npts; L.n[a] = o->n_line[a]; L.n_le[a] = o->n_le[a]; L.i_ge[a] = o->i_ge[a];
        npts += o->n_line[a];
    }
    L.factor[0] = o->beam_factor[0]; L.factor[1] = o->beam_factor[1];
    if (npts > 0 && !line_pts) return fail(c, OLX_EINVAL, "olx_solution_analyze: line points missing");
    for (int a = 0; a < 3; ++a) if (!(o->aspect[a] != 0.0)) return fail(c, OLX_EINVAL, "olx_solution_analyze: zero aspect ratio");
    HIPCHK(c, hipSetDevice(c->device));
    // device / pinned layout.  in: [A 12 F f64][pts 3 npts F f64][weights F f32]   out: [peaks 6 F u32][ita F + 1 u32][bounds 12 F i32][moments 4 F f64]
    // work (device only): [cut F f32][samples npts F f32]
    auto up8 = [](size_t v) { return (v + 7) & ~(size_t)7; };
    const size_t in_A = 0, in_pts = in_A + sizeof(double) * 12 * F, in_w = in_pts + sizeof(double) * 3 * (size_t)npts * F;
    const size_t in_box = in_w + sizeof(float) * F, in_sc = in_box + sizeof(int) * 6 * F, in_bytes = up8(in_sc + sizeof(float) * F);
    const size_t out_pk = in_bytes, out_ita = out_pk + sizeof(unsigned) * 6 * F, out_bd = out_ita + sizeof(unsigned) * (F + 1);
    const size_t out_mom = up8(out_bd + sizeof(int) * 12 * F), out_end = out_mom + sizeof(double) * 4 * F;
    const size_t wk_cut = out_end, wk_smp = up8(wk_cut + sizeof(float) * F), dev_bytes = wk_smp + sizeof(float) * (size_t)npts * F + 8;
    { int rc = analysis_scratch(c, dev_bytes, out_end); if (rc) return rc; }
    { int rc = c->d_wint.reserve(c, (size_t)c->fp.vox); if (rc) return rc; }
    unsigned char* h = static_cast<unsigned char*>(c->h_an);
    unsigned char* d = c->d_an;
    memcpy(h + in_A, A, sizeof(double) * 12 * F);
    if (npts) memcpy(h + in_pts, line_pts, sizeof(double) * 3 * (size_t)npts * F);
    for (int f = 0; f < F; ++f) reinterpret_cast<float*>(h + in_w)[f] = (float)ita_weights[f];
    focus_boxes(c, A, o->aspect, o->r_main_m, F, reinterpret_cast<int*>(h + in_box));     // the mainlobe ellipsoids' index boxes
    const int* d_box = reinterpret_cast<const int*>(d + in_box);
    const bool quad = (c->fp.nz & 3) == 0 && c->fp.vox < (1ll << 33);
    // scale_per_focus given: Solution.scale and the aggregation over foci happen first -- fused with the peak scan and the
    // time-average volume into ONE pass over the volumes when the shape allows (<= 8 foci, z rows of whole quads, no complex output),
    // otherwise as the separate olx_field_scale_aggregate pass
    const bool rowquads = (long long)c->fp.nx * c->fp.ny * ((c->fp.nz + 3) / 4) < (1ll << 31);      // (the fused pass walks ROW quads: rows of any length)
    const bool fused = scale_per_focus && rowquads && F <= SAA_MAXF && !(c->flags & OLX_OUT_COMPLEX);
    if (scale_per_focus && !fused) { int rc = olx_field_scale_aggregate(c, scale_per_focus, F); if (rc) return rc; }
    if (fused) {
        { int rc_ = exported_buffers_quiesce(c, c->cur); if (rc_) return rc_; }   // (p2p: the fused pass scales the volumes in place)
        { int rc_ = aggregate_buffers_free(c); if (rc_) return rc_; }
        { int rc_ = reserve_aggregate(c, true, true); if (rc_) return rc_; }
        for (int f = 0; f < F; ++f) reinterpret_cast<float*>(h + in_sc)[f] = (float)scale_per_focus[f];
    }
    HIPCHK(c, hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(d + out_pk, 0, out_end - out_pk, c->stream));
    const double* d_A = reinterpret_cast<const double*>(d + in_A);
    unsigned* d_pk = reinterpret_cast<unsigned*>(d + out_pk);
    unsigned* d_ita = reinterpret_cast<unsigned*>(d + out_ita);
    float* d_cut = reinterpret_cast<float*>(d + wk_cut);
    float* d_smp = reinterpret_cast<float*>(d + wk_smp);
    const float* pm = c->d_pmag[c->cur];
    PeakParams P; fill_scan_params(c, P, o->aspect);
    // (1) the six masked peaks of |p| and intensity, one pass
    P.radius = o->r_main_m; P.op = 0; P.use_zmin = 1; P.zmin = o->zmin_m;
    const long long want = (P.vox + 255) / 256;
    const bool D = c->derive_i; const float IK_ = c->fp.inten_scale;      // (a deriving plan: every intensity below is olx_inten of the |p| the scan loads)
    if (fused)      // scale + aggregate + peaks + time-average volume (with its global peak) in one pass
        hipLaunchKernelGGL(saa_kernel(c), dim3(2048), dim3(256), 0, c->stream, c->d_pmag[c->cur], inten_arg(c), reinterpret_cast<const float*>(d + in_sc),
                           reinterpret_cast<const float*>(d + in_w), d_A, F, P, o->r_side_m, 1.0f / (float)F, IK_, c->d_agg_p, c->d_agg_i, c->d_wint, d_pk, d_ita + F);
    if (fused) { c->inten_live = false; int rc_ = pmax_post(c, reinterpret_cast<const float*>(d + in_sc), true); if (rc_) return rc_; }
    else if (quad) hipLaunchKernelGGL(D ? field_analysis_peaks4_k<true> : field_analysis_peaks4_k<false>, dim3(scan_blocks(want, F), F), dim3(256), 0, c->stream, pm, inten_arg(c), d_A, P, o->r_side_m, IK_, d_pk);
    else hipLaunchKernelGGL(D ? field_analysis_peaks_k<true> : field_analysis_peaks_k<false>, dim3((unsigned)std::min<long long>(want, 2048), F), dim3(256), 0, c->stream, pm, inten_arg(c), d_A, P, o->r_side_m, IK_, d_pk);
    // (2) -3 dB centroid of the mainlobe: cut-off from the peak just found
    hipLaunchKernelGGL(analysis_cutoffs_k, dim3((F + 63) / 64), dim3(64), 0, c->stream, d_pk, F, o->centroid_factor, d_cut);
    P.use_zmin = 0; P.zmin = 0;
    hipLaunchKernelGGL(field_masked_moments_box_k, dim3(32, F), dim3(256), 0, c->stream, pm, d_A, d_cut, P, d_box, reinterpret_cast<double*>(d + out_mom));
    // (3) time-average intensity volume, its mainlobe peaks (F masks over the ONE volume) and its global peak above zmin
    P.zmin = o->zmin_m;        // (the global peak above zmin comes out of the same pass that writes the volume)
    if (!fused) hipLaunchKernelGGL(D ? field_weighted_sum_peak_k<true> : field_weighted_sum_peak_k<false>, dim3(2048), dim3(256), 0, c->stream, D ? pm : (const float*)c->d_inten, reinterpret_cast<const float*>(d + in_w), F, P, IK_, c->d_wint, d_ita + F);
    P.vol_stride = 0; P.zmin = 0;
    hipLaunchKernelGGL(field_masked_peak_box_k, dim3(32, F), dim3(256), 0, c->stream, c->d_wint, d_A, P, d_box, d_ita);
    // (4) beam widths: |p| along the three focal axes of every focus, then the cut-off crossings
    if (npts) {
        P.vol_stride = c->fp.vox;
        hipLaunchKernelGGL(field_sample_lines_k, dim3((npts + 127) / 128, F), dim3(128), 0, c->stream, pm, reinterpret_cast<const double*>(d + in_pts), npts, P, d_smp);
        hipLaunchKernelGGL(beam_bounds_k, dim3(3, F), dim3(64), 0, c->stream, d_smp, npts, d_pk, L, reinterpret_cast<int*>(d + out_bd));
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h + out_pk, d + out_pk, out_end - out_pk, hipMemcpyDeviceToHost, c->stream));
    // everything is enqueued; the report sits in the pinned block once the stream has drained (olx_solution_analyze_finish)
    c->an_pending = true; c->an_F = F; c->an_npts = npts; c->an_out_pk = out_pk; c->an_out_ita = out_ita; c->an_out_bd = out_bd; c->an_out_mom = out_mom;
    return OLX_OK;
}

int olx_solution_analyze_finish(olx_ctx* c, olx_focus_report* reports, float* ita_global) {
    if (!c) return OLX_EINVAL;
    if (!reports || !ita_global) return fail(c, OLX_EINVAL, "olx_solution_analyze_finish: null argument");
    if (!c->an_pending) return fail(c, OLX_ESTATE, "olx_solution_analyze_finish: no analysis in flight (olx_solution_analyze_begin first)");
    c->an_pending = false;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const unsigned char* h = static_cast<const unsigned char*>(c->h_an);
    const int F = c->an_F, npts = c->an_npts;
    const size_t out_pk = c->an_out_pk, out_ita = c->an_out_ita, out_bd = c->an_out_bd, out_mom = c->an_out_mom;
    const float* pk = reinterpret_cast<const float*>(h + out_pk);
    const float* ita = reinterpret_cast<const float*>(h + out_ita);
    const int* bd = reinterpret_cast<const int*>(h + out_bd);
    const double* mom = reinterpret_cast<const double*>(h + out_mom);
    for (int f = 0; f < F; ++f) {
        olx_focus_report& R = reports[f];
        for (int k = 0; k < 6; ++k) R.peaks[k] = pk[6 * f + k];
        R.ita_main = ita[f]; R.reserved = 0.f;
        for (int k = 0; k < 4; ++k) R.moments[k] = mom[4 * f + k];
        for (int k = 0; k < 12; ++k) (&R.bounds[0][0][0])[k] = npts ? bd[12 * f + k] : -1;
    }
    *ita_global = ita[F];
    return OLX_OK;
}

int olx_solution_analyze(olx_ctx* c, const double* A, const double* ita_weights, const double* line_pts,
                         const olx_analysis_opts* o, const double* scale_per_focus, olx_focus_report* reports, float* ita_global) {
    if (c && (!reports || !ita_global)) return fail(c, OLX_EINVAL, "olx_solution_analyze: null argument");
    const int rc = olx_solution_analyze_begin(c, A, ita_weights, line_pts, o, scale_per_focus);
    return rc ? rc : olx_solution_analyze_finish(c, reports, ita_global);
}

// RCCL prints a version banner through C stdio on stdout; callers (bench.py) own stdout for their
// one-line JSON, so stdout is pointed at stderr while RCCL initialises and flushed before restoring.
struct StdoutToStderr {
    int saved;
    StdoutToStderr() { fflush(stdout); saved = dup(1); if (saved >= 0) dup2(2, 1); }
    ~StdoutToStderr() { fflush(stdout); if (saved >= 0) { dup2(saved, 1); close(saved); } }
};

// ---- RCCL reassembly ------------------------------------------------------------------------
static int load_rccl(olx_ctx* c) {
    RcclApi& r = c->rccl;
    if (r.handle) return OLX_OK;
    // The system ROCm's RCCL first: libolx.so is built against and runs on /opt/rocm's HIP runtime; a bare "librccl.so.1"
    // can resolve to another ROCm build earlier on the search path (e.g. the copy bundled with a PyTorch wheel in the
    // launcher's process).  OLX_RCCL_PATH overrides; olx_rccl_path() reports what was bound.
    const char* envp = getenv("OLX_RCCL_PATH");
    const char* names[] = {envp ? envp : "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so", "librccl.so.1", "librccl.so"};
    for (const char* nm : names) { r.handle = dlopen(nm, RTLD_NOW | RTLD_LOCAL); if (r.handle) break; }
    if (!r.handle) return fail(c, OLX_ECOMM, "RCCL not found: %s", dlerror());
    r.GetUniqueId = (int (*)(olx_nccl_id*))dlsym(r.handle, "ncclGetUniqueId");
    r.CommInitRank = (int (*)(olx_nccl_comm*, int, olx_nccl_id, int))dlsym(r.handle, "ncclCommInitRank");
    r.CommDestroy = (int (*)(olx_nccl_comm))dlsym(r.handle, "ncclCommDestroy");
    r.AllGather = (int (*)(const void*, void*, size_t, int, olx_nccl_comm, hipStream_t))dlsym(r.handle, "ncclAllGather");
    r.GetErrorString = (const char* (*)(int))dlsym(r.handle, "ncclGetErrorString");
    r.AllReduce = (int (*)(const void*, void*, size_t, int, int, olx_nccl_comm, hipStream_t))dlsym(r.handle, "ncclAllReduce");
    r.ReduceScatter = (int (*)(const void*, void*, size_t, int, int, olx_nccl_comm, hipStream_t))dlsym(r.handle, "ncclReduceScatter");  // optional
    r.CommCount = (int (*)(olx_nccl_comm, int*))dlsym(r.handle, "ncclCommCount");  // optional
    if (!r.GetUniqueId || !r.CommInitRank || !r.CommDestroy || !r.AllGather || !r.AllReduce || !r.GetErrorString)
        return fail(c, OLX_ECOMM, "RCCL symbols missing");
    Dl_info info;
    c->rccl_path = (dladdr((void*)r.AllGather, &info) && info.dli_fname) ? info.dli_fname : "(unknown)";
    return OLX_OK;
}
#define NCCLCHK(c, call)                                                                              \
    do {                                                                                              \
        int r_ = (call);                                                                              \
        if (r_ != 0) return fail((c), OLX_ECOMM, "%s: %s", #call, (c)->rccl.GetErrorString(r_));      \
    } while (0)

const char* olx_rccl_path(const olx_ctx* c) { return c ? c->rccl_path.c_str() : ""; }

int olx_comm_unique_id(olx_ctx* c, void* id_bytes) {
    if (!c || !id_bytes) return OLX_EINVAL;
    if (olx_p2p_requested()) return olx_p2p_unique_id(c, id_bytes);     // OLX_GATHER=p2p: the id names the transport's control block
    int rc = load_rccl(c);
    if (rc) return rc;
    olx_nccl_id id;
    StdoutToStderr quiet;
    NCCLCHK(c, c->rccl.GetUniqueId(&id));
    memcpy(id_bytes, &id, sizeof id);
    return OLX_OK;
}

int olx_comm_init(olx_ctx* c, const void* id_bytes, int nranks, int rank) {
    if (!c || !id_bytes) return OLX_EINVAL;
    if (nranks < 1 || rank < 0 || rank >= nranks) return fail(c, OLX_EINVAL, "olx_comm_init: bad rank %d / %d", rank, nranks);
    if (c->comm || (c->p2p && c->comm_stream)) return fail(c, OLX_ESTATE, "olx_comm_init: communicator already initialised");
    HIPCHK(c, hipSetDevice(c->device));
    if (olx_p2p_is_id(id_bytes)) {      // rank 0 chose the peer-to-peer transport: no RCCL at all
        int rc = olx_p2p_init(c, id_bytes, nranks, rank);
        if (rc) return rc;
        c->nranks = nranks; c->rank = rank;
        HIPCHK(c, hipStreamCreateWithFlags(&c->comm_stream, hipStreamNonBlocking));
        for (int b = 0; b < olx_ctx::NBUF; ++b) {
            HIPCHK(c, hipEventCreateWithFlags(&c->ev_field[b], hipEventDisableTiming));
            HIPCHK(c, hipEventCreateWithFlags(&c->ev_gather[b], hipEventDisableTiming));
        }
        c->planned = false;
        return OLX_OK;
    }
    int rc = load_rccl(c);
    if (rc) return rc;
    olx_nccl_id id;
    memcpy(&id, id_bytes, sizeof id);
    {
        StdoutToStderr quiet;
        NCCLCHK(c, c->rccl.CommInitRank(&c->comm, nranks, id, rank));
    }
    c->nranks = nranks; c->rank = rank;
    HIPCHK(c, hipStreamCreateWithFlags(&c->comm_stream, hipStreamNonBlocking));
    for (int b = 0; b < olx_ctx::NBUF; ++b) {
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_field[b], hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_gather[b], hipEventDisableTiming));
    }
    c->planned = false;  // re-plan to get double-buffered outputs
    return OLX_OK;
}

int olx_comm_destroy(olx_ctx* c) {
    if (!c) return OLX_EINVAL;
    if (c->p2p) {   // (the peers' mappings of this rank's blocks outlive the communicator only until the blocks are freed: wait for their pulls first;
        hipSetDevice(c->device);                    // best effort -- a peer that is gone shows up as a timeout, and the teardown goes on)
        (void)exported_buffers_quiesce(c, -1);
        olx_p2p_destroy(c);
    }
    if (c->comm_stream) hipStreamSynchronize(c->comm_stream);
    if (c->comm) { c->rccl.CommDestroy(c->comm); c->comm = nullptr; }
    for (int b = 0; b < olx_ctx::NBUF; ++b) {
        if (c->ev_field[b]) { hipEventDestroy(c->ev_field[b]); c->ev_field[b] = nullptr; }
        if (c->ev_gather[b]) { hipEventDestroy(c->ev_gather[b]); c->ev_gather[b] = nullptr; }
        c->gather_pending[b] = false;
    }
    if (c->ev_agg) { hipEventDestroy(c->ev_agg); hipEventDestroy(c->ev_red); c->ev_agg = c->ev_red = nullptr; }
    c->reduce_pending = false;
    if (c->comm_stream) { hipStreamDestroy(c->comm_stream); c->comm_stream = nullptr; }
    c->nranks = 1; c->rank = 0;
    return OLX_OK;
}

// p2p transport only: after EVERY olx_field_plan each rank exports the IPC handles of its output blocks, the launcher
// all-gathers the blobs (rank order) and every rank imports them
int olx_comm_export(olx_ctx* c, void* blob_out) {
    if (!c || !blob_out) return OLX_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return olx_p2p_export(c, blob_out);
}
int olx_comm_import(olx_ctx* c, const void* blobs) {
    if (!c || !blobs) return OLX_EINVAL;
    return olx_p2p_import(c, blobs);
}
const char* olx_comm_transport(const olx_ctx* c) { return !c ? "" : c->p2p ? "p2p" : c->comm ? "rccl" : ""; }
int olx_comm_ranks_seen(olx_ctx* c) {
    if (!c) return OLX_EINVAL;
    if (c->p2p) return olx_p2p_attached(c);
    if (c->comm && c->rccl.CommCount) { int n = 0; NCCLCHK(c, c->rccl.CommCount(c->comm, &n)); return n; }
    return c->comm ? c->nranks : 0;
}

int olx_field_allgather(olx_ctx* c) {
    if (!c) return OLX_EINVAL;
    if (!c->comm_active()) return fail(c, OLX_ESTATE, "olx_field_allgather: call olx_comm_init first");
    if (!c->planned) return fail(c, OLX_ESTATE, "olx_field_allgather: nothing planned");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->p2p) return olx_p2p_allgather(c);
    const size_t count = (size_t)c->fp.vox * c->plan_foci;
    const size_t need = count * c->nranks;
    if (c->d_gather.capacity() < need) {
        HIPCHK(c, hipStreamSynchronize(c->comm_stream));     // (an earlier gather may still write the block)
        int rc = c->d_gather.reserve(c, need);
        if (rc) return rc;
    }
    const int b = c->cur;
    HIPCHK(c, hipEventRecord(c->ev_field[b], c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->comm_stream, c->ev_field[b], 0));
    NCCLCHK(c, c->rccl.AllGather(c->d_pmag[b], c->d_gather, count, kNcclFloat32, c->comm, c->comm_stream));
    HIPCHK(c, hipEventRecord(c->ev_gather[b], c->comm_stream));
    c->gather_pending[b] = true;
    return OLX_OK;
}

// Aggregated result across ranks (plan/protocol.py:382-387 with the foci sharded over GPUs): local
// max / sum over this rank's foci on the compute stream, then RCCL all-reduce (max for |p|, sum for the
// intensity mean) of ONE volume each on the side stream -- the exchange step the sharded path really has.
static int aggregate_exchange(olx_ctx* c, bool want_scatter) {
    if (!c) return OLX_EINVAL;
    if (!c->comm && !c->p2p) return fail(c, OLX_ESTATE, "olx_field_allreduce_aggregate / olx_field_reduce_scatter_aggregate: call olx_comm_init first");
    if (!c->planned) return fail(c, OLX_ESTATE, "olx_field_allreduce_aggregate: nothing planned");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t vox = (size_t)c->fp.vox;
    const bool with_i = (c->flags & OLX_OUT_INTENSITY) != 0;
    { int rc = reserve_aggregate(c, true, with_i); if (rc) return rc; }
    if (!c->ev_agg) { HIPCHK(c, hipEventCreateWithFlags(&c->ev_agg, hipEventDisableTiming)); HIPCHK(c, hipEventCreateWithFlags(&c->ev_red, hipEventDisableTiming)); }
    { int rc = aggregate_buffers_free(c); if (rc) return rc; }   // the previous exchange still owns the aggregate buffers
    // genuine foci of this rank come first in its shard (padding repeats the last one, dist.plan_foci_orbits): only they enter
    // the local max / sum, and the mean divides by the GLOBAL number of genuine foci (olx_field_aggregate_counts)
    const int n_local = c->agg_local >= 0 ? std::min(c->agg_local, c->plan_foci) : c->plan_foci;
    const float inv_n = 1.0f / (c->agg_total > 0 ? (float)c->agg_total : (float)c->plan_foci * (float)c->nranks);
    if (!c->uploaded && !c->derive_i && (vox & 3) == 0)   // launched result with stored volumes: intensity == scale(v) |p|^2, aggregate from |p| alone (half the reads);
                                                            // a deriving plan takes field_aggregate_k's DERIVE form below: also |p| alone, and the bits of the single-rank aggregate
        hipLaunchKernelGGL(field_aggregate_p_k, dim3(4096), dim3(256), 0, c->stream, c->d_pmag[c->cur], n_local, (long long)vox,
                           inv_n, c->fp.inten_scale, c->hetero ? (const float*)c->d_inv2z : (c->pulsed && c->pulse_med && c->pm_has_z ? (const float*)c->d_pm_inv2z : nullptr), c->d_agg_p, with_i ? c->d_agg_i : nullptr);
    else
        hipLaunchKernelGGL(c->derive_i ? field_aggregate_k<true> : field_aggregate_k<false>, dim3(2048), dim3(256), 0, c->stream, c->d_pmag[c->cur], with_i ? inten_arg(c) : nullptr,
                           n_local, (long long)vox, inv_n, c->fp.inten_scale, c->d_agg_p, with_i ? c->d_agg_i : nullptr);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev_agg, c->stream));
    if (c->p2p)     // peer-to-peer transport: the same two shapes, pulled slice by slice over IPC mappings (csrc/olx_p2p.hip)
        return olx_p2p_aggregate(c, want_scatter && vox % ((size_t)4 * c->nranks) == 0, with_i);
    HIPCHK(c, hipStreamWaitEvent(c->comm_stream, c->ev_agg, 0));
    // Exchange.  Reduce-scatter (in place): rank r ends up owning voxels [r vox/N, (r+1) vox/N) of the global aggregate
    // (max |p|, mean intensity), i.e. the result stays sharded in HBM like the per-focus volumes; that moves (N-1)/N of
    // one volume pair per rank, half of an all-reduce.  All-reduce replicates the whole aggregate on every rank; it is
    // also the fallback when the voxel count does not divide by N.
    const bool scatter = want_scatter && c->rccl.ReduceScatter && vox % (size_t)c->nranks == 0;
    if (scatter) {
        const size_t chunk = vox / (size_t)c->nranks;
        NCCLCHK(c, c->rccl.ReduceScatter(c->d_agg_p, c->d_agg_p + chunk * c->rank, chunk, kNcclFloat32, kNcclMax, c->comm, c->comm_stream));
        if (with_i) NCCLCHK(c, c->rccl.ReduceScatter(c->d_agg_i, c->d_agg_i + chunk * c->rank, chunk, kNcclFloat32, kNcclSum, c->comm, c->comm_stream));
    } else {
        NCCLCHK(c, c->rccl.AllReduce(c->d_agg_p, c->d_agg_p, vox, kNcclFloat32, kNcclMax, c->comm, c->comm_stream));
        if (with_i) NCCLCHK(c, c->rccl.AllReduce(c->d_agg_i, c->d_agg_i, vox, kNcclFloat32, kNcclSum, c->comm, c->comm_stream));
    }
    HIPCHK(c, hipEventRecord(c->ev_red, c->comm_stream));
    c->reduce_pending = true;
    return OLX_OK;
}

int olx_field_aggregate_counts(olx_ctx* c, int local_valid, int global_total) {
    if (!c) return OLX_EINVAL;
    if (local_valid < 0 || global_total < 1) return fail(c, OLX_EINVAL, "olx_field_aggregate_counts: need local_valid >= 0 and global_total >= 1");
    c->agg_local = local_valid; c->agg_total = global_total;
    return OLX_OK;
}

int olx_field_allreduce_aggregate(olx_ctx* c) { return aggregate_exchange(c, false); }
int olx_field_reduce_scatter_aggregate(olx_ctx* c) { return aggregate_exchange(c, true); }

int olx_aggregate_fetch(olx_ctx* c, float* pmax_out, float* imean_out) {
    if (!c) return OLX_EINVAL;
    if (!c->d_agg_p) return fail(c, OLX_ESTATE, "olx_aggregate_fetch: no aggregate computed");
    if (imean_out && !c->d_agg_i) return fail(c, OLX_ESTATE, "olx_aggregate_fetch: intensity not aggregated");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->comm_stream) HIPCHK(c, hipStreamSynchronize(c->comm_stream));
    if (c->p2p) { int rc = olx_p2p_drain(c); if (rc) return rc; }
    const size_t vox = (size_t)c->fp.vox;
    int rc = OLX_OK;
    if (pmax_out) rc = fetch_to_host(c, pmax_out, c->d_agg_p, sizeof(float) * vox);      // (pipelined staged copy, as the per-focus fetches)
    if (!rc && imean_out) rc = fetch_to_host(c, imean_out, c->d_agg_i, sizeof(float) * vox);
    return rc;
}

int olx_aggregate_fetch_pmax(olx_ctx* c, float* pmax_out) {
    if (!c) return OLX_EINVAL;
    if (!pmax_out) return fail(c, OLX_EINVAL, "olx_aggregate_fetch_pmax: null output");
    if (!c->agg_pmax_valid) return fail(c, OLX_ESTATE, "olx_aggregate_fetch_pmax: no aggregate of p_max volumes (aggregate a launched pulsed plan with OLX_OUT_PMAX first)");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return fetch_to_host(c, pmax_out, c->d_agg_pmax, sizeof(float) * (size_t)c->fp.vox);
}

int olx_allgather_fetch(olx_ctx* c, int rank, float* out) {
    if (!c || !out) return OLX_EINVAL;
    if (!c->d_gather) return fail(c, OLX_ESTATE, "olx_allgather_fetch: no gather issued");
    if (rank < 0 || rank >= c->nranks) return fail(c, OLX_EINVAL, "olx_allgather_fetch: rank out of range");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->comm_stream));
    if (c->p2p) { int rc = olx_p2p_drain(c); if (rc) return rc; }
    const size_t count = (size_t)c->fp.vox * c->plan_foci;
    return fetch_to_host(c, out, c->d_gather + count * rank, sizeof(float) * count);
}

}  // extern "C"

// ---- thermal model (kernel 3, k_thermal.hip) ---------------------------------------------------------------------------------------
extern "C" {

int olx_thermal_plan(olx_ctx* c, const olx_grid* g, const float* density, const float* specific_heat, const float* conductivity,
                     const float* absorption, double density0, double specific_heat0, double conductivity0, double absorption0,
                     double perfusion, double* dt_max_out) {
    if (!c) return OLX_EINVAL;
    if (!g) return fail(c, OLX_EINVAL, "olx_thermal_plan: null grid");
    for (int a = 0; a < 3; ++a)
        if (g->n[a] < 1 || !(g->spacing[a] > 0) || !std::isfinite(g->spacing[a])) return fail(c, OLX_EINVAL, "olx_thermal_plan: bad grid axis %d", a);
    if ((!density && !(density0 > 0)) || (!specific_heat && !(specific_heat0 > 0)) || (!conductivity && !(conductivity0 > 0)) ||
        (!absorption && !(absorption0 >= 0)) || !(perfusion >= 0) || !std::isfinite(perfusion))
        return fail(c, OLX_EINVAL, "olx_thermal_plan: the scalars of NULL volumes must be > 0 (absorption >= 0) and perfusion finite and >= 0");
    {   // the volumes that are given: the pack kernel's maximum drops a NaN rate and a negative one loses to any sane lane of its wave
        const float* vol[4] = {density, specific_heat, conductivity, absorption};
        const char* what[4] = {"density", "specific heat", "conductivity", "absorption"};
        const size_t nvox = (size_t)g->n[0] * g->n[1] * g->n[2];
        for (int q = 0; q < 4; ++q) {
            if (!vol[q]) continue;
            const size_t o = olxmed::first_bad(vol[q], nvox, q == 3 ? olxmed::NON_NEGATIVE : olxmed::POSITIVE);
            if (o < nvox) return fail(c, OLX_EINVAL, "olx_thermal_plan: %s must be finite and %s (voxel %zu)", what[q], q == 3 ? ">= 0" : "> 0", o);
        }
    }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    ThermalParams& P = c->th;
    P = ThermalParams{};
    P.nx = g->n[0]; P.ny = g->n[1]; P.nz = g->n[2];
    P.vox = (long long)P.nx * P.ny * P.nz;
    P.ihx2 = (float)(1.0 / (g->spacing[0] * g->spacing[0]));
    P.ihy2 = (float)(1.0 / (g->spacing[1] * g->spacing[1]));
    P.ihz2 = (float)(1.0 / (g->spacing[2] * g->spacing[2]));
    P.rho0 = (float)density0; P.cp0 = (float)specific_heat0; P.kappa0 = (float)conductivity0; P.alpha0 = (float)absorption0;
    P.perf = (float)perfusion;
    c->th_uniform = !density && !specific_heat && !conductivity && !absorption;
    const size_t vox = (size_t)P.vox;
    for (DevBuf<float>* b : {&c->d_th_T[0], &c->d_th_T[1], &c->d_th_max, &c->d_th_cem}) { int rc = b->reserve(c, vox); if (rc) return rc; }
    { int rc = c->d_th_rate.reserve(c, 1); if (rc) return rc; }
    if (c->th_uniform) {
        const double rc = density0 * specific_heat0;
        P.gx = (float)(conductivity0 * P.ihx2); P.gy = (float)(conductivity0 * P.ihy2); P.gz = (float)(conductivity0 * P.ihz2);
        P.irc0 = (float)(1.0 / rc); P.sfac0 = (float)(2.0 * absorption0 * 1e4 / rc);
        const double ih2 = 1.0 / (g->spacing[0] * g->spacing[0]) + 1.0 / (g->spacing[1] * g->spacing[1]) + 1.0 / (g->spacing[2] * g->spacing[2]);
        c->th_rate = (2.0 * conductivity0 * ih2 + perfusion) / rc;
    } else {
        // the four volumes (or their scalars) go up once, the pack kernel forms the coefficients, the volumes are freed again
        DevScratch scr;
        const float* src[4] = {density, specific_heat, conductivity, absorption};
        size_t nvol = 0;
        for (const float* p : src) nvol += p ? 1 : 0;
        HIPCHK(c, hipMalloc(&scr.p, sizeof(float) * vox * std::max(nvol, (size_t)1)));
        const float* dv[4] = {nullptr, nullptr, nullptr, nullptr};
        size_t at = 0;
        for (int q = 0; q < 4; ++q) {
            if (!src[q]) continue;
            float* d = scr.at<float>(sizeof(float) * vox * at++);
            HIPCHK(c, hipMemcpy(d, src[q], sizeof(float) * vox, hipMemcpyHostToDevice));
            dv[q] = d;
        }
        int rc = c->d_th_coef.reserve(c, vox);
        if (!rc) rc = c->d_th_irc.reserve(c, vox);
        if (!rc) rc = c->d_th_sfac.reserve(c, vox);
        if (rc) return rc;
        HIPCHK(c, hipMemsetAsync(c->d_th_rate, 0, sizeof(unsigned), c->stream));
        olx_thermal_pack(c, dv[0], dv[1], dv[2], dv[3]);
        HIPCHK(c, hipGetLastError());
        unsigned bits = 0;
        HIPCHK(c, hipMemcpyAsync(&bits, c->d_th_rate, sizeof bits, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        float rate;
        memcpy(&rate, &bits, sizeof rate);
        c->th_rate = rate;
    }
    if (!(c->th_rate > 0) || !std::isfinite(c->th_rate)) return fail(c, OLX_EINVAL, "olx_thermal_plan: the medium gives no finite FTCS bound");
    if (dt_max_out) *dt_max_out = 1.0 / c->th_rate;
    c->th_planned = true;
    c->th_steps = 0; c->th_npts = 0; c->th_next = -1;
    c->th_src_foci = 0; c->th_src_resident = false; c->th_src_pii = false;
    return OLX_OK;
}

int olx_thermal_schedule(olx_ctx* c, int n_steps, const int* row_ptr, const int* focus, const double* tau_s, int n_points, const long long* points) {
    if (!c) return OLX_EINVAL;
    if (!c->th_planned) return fail(c, OLX_ESTATE, "olx_thermal_schedule: no thermal plan");
    if (n_steps < 1 || !row_ptr || n_points < 0 || (n_points > 0 && !points)) return fail(c, OLX_EINVAL, "olx_thermal_schedule: n_steps < 1, null row_ptr or bad points");
    if (row_ptr[0] != 0) return fail(c, OLX_EINVAL, "olx_thermal_schedule: row_ptr[0] must be 0");
    for (int n = 0; n < n_steps; ++n)
        if (row_ptr[n + 1] < row_ptr[n]) return fail(c, OLX_EINVAL, "olx_thermal_schedule: row_ptr must not decrease");
    const int ne = row_ptr[n_steps];
    if (ne > 0 && (!focus || !tau_s)) return fail(c, OLX_EINVAL, "olx_thermal_schedule: null focus / tau");
    std::vector<float> tau(ne);
    int fmax = -1;
    for (int e = 0; e < ne; ++e) {
        fmax = std::max(fmax, focus[e]);
        if (focus[e] < 0) return fail(c, OLX_EINVAL, "olx_thermal_schedule: negative focus index");
        if (!(tau_s[e] >= 0) || !std::isfinite(tau_s[e])) return fail(c, OLX_EINVAL, "olx_thermal_schedule: on-times must be finite and >= 0");
        tau[e] = (float)tau_s[e];
    }
    for (int p = 0; p < n_points; ++p)
        if (points[p] < 0 || points[p] >= c->th.vox) return fail(c, OLX_EINVAL, "olx_thermal_schedule: trace point %d outside the grid", p);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int rc = c->d_th_sf.reserve(c, ne);
    if (!rc) rc = c->d_th_tau.reserve(c, ne);
    if (!rc) rc = c->d_th_pts.reserve(c, n_points);
    if (!rc) rc = c->d_th_trace.reserve(c, (size_t)n_steps * n_points);
    if (rc) return rc;
    if (ne > 0) {
        HIPCHK(c, hipMemcpy(c->d_th_sf, focus, sizeof(int) * ne, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(c->d_th_tau, tau.data(), sizeof(float) * ne, hipMemcpyHostToDevice));
    }
    if (n_points > 0) HIPCHK(c, hipMemcpy(c->d_th_pts, points, sizeof(long long) * n_points, hipMemcpyHostToDevice));
    c->th_row.assign(row_ptr, row_ptr + n_steps + 1);
    c->th_steps = n_steps; c->th_npts = n_points; c->th_next = -1; c->th_max_focus = fmax;
    return OLX_OK;
}

int olx_thermal_source(olx_ctx* c, int n_foci, const float* intensity) {
    if (!c) return OLX_EINVAL;
    if (!c->th_planned) return fail(c, OLX_ESTATE, "olx_thermal_source: no thermal plan");
    if (n_foci < 1) return fail(c, OLX_EINVAL, "olx_thermal_source: n_foci < 1");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (intensity) {
        const size_t total = (size_t)c->th.vox * n_foci;
        { int rc_ = c->d_th_I.reserve(c, total); if (rc_) return rc_; }
        HIPCHK(c, hipMemcpy(c->d_th_I, intensity, sizeof(float) * total, hipMemcpyHostToDevice));
        c->th_src_resident = false;
    } else {
        c->th_src_resident = true;     // checked against the resident result at every olx_thermal_run
    }
    c->th_src_foci = n_foci; c->th_src_pii = false;
    return OLX_OK;
}

int olx_thermal_source_pii(olx_ctx* c, int n_foci) {
    if (!c) return OLX_EINVAL;
    if (!c->th_planned) return fail(c, OLX_ESTATE, "olx_thermal_source_pii: no thermal plan");
    if (!c->pii_live) return fail(c, OLX_ESTATE, "olx_thermal_source_pii: no resident pulse intensity integrals (a launched pulsed plan with OLX_OUT_PII, or olx_pii_upload)");
    if (n_foci != c->pii_foci) return fail(c, OLX_EINVAL, "olx_thermal_source_pii: %d foci given, the resident pulse intensity integrals have %d", n_foci, c->pii_foci);
    c->th_src_resident = true; c->th_src_pii = true;     // checked against the resident volumes at every olx_thermal_run
    c->th_src_foci = n_foci;
    return OLX_OK;
}

int olx_thermal_run(olx_ctx* c, double dt, double baseline, int first_step, int n_steps) {
    if (!c) return OLX_EINVAL;
    if (!c->th_planned || c->th_steps < 1 || c->th_src_foci < 1) return fail(c, OLX_ESTATE, "olx_thermal_run: needs olx_thermal_plan, _schedule and _source first");
    if (!(dt > 0) || !std::isfinite(dt) || !std::isfinite(baseline)) return fail(c, OLX_EINVAL, "olx_thermal_run: dt must be finite and > 0, baseline finite");
    if (dt * c->th_rate > 1.0 + 1e-5) return fail(c, OLX_EINVAL, "olx_thermal_run: dt = %g s is above the FTCS bound %g s", dt, 1.0 / c->th_rate);
    if (n_steps < 0 || first_step < 0 || first_step + n_steps > c->th_steps) return fail(c, OLX_EINVAL, "olx_thermal_run: steps [%d, %d) outside the schedule's %d", first_step, first_step + n_steps, c->th_steps);
    if (first_step > 0 && first_step != c->th_next) return fail(c, OLX_ESTATE, "olx_thermal_run: step %d does not continue the last run (next step %d)", first_step, c->th_next);
    const float* inten = c->d_th_I;
    if (c->th_src_resident && c->th_src_pii) {
        const bool whole = c->planned && c->pii_live && c->d_pii && c->slab.x_begin == 0 && c->slab.x_count == c->grid.n[0] &&
                           c->grid.n[0] == c->th.nx && c->grid.n[1] == c->th.ny && c->grid.n[2] == c->th.nz && c->pii_foci == c->th_src_foci;
        if (!whole) return fail(c, OLX_ESTATE, "olx_thermal_run: no resident whole-grid pulse intensity integrals of %d foci on the thermal grid", c->th_src_foci);
        inten = c->d_pii;
    } else if (c->th_src_resident) {
        const bool whole = c->planned && (c->d_inten || c->derive_i) && (c->flags & OLX_OUT_INTENSITY) && c->slab.x_begin == 0 && c->slab.x_count == c->grid.n[0] &&
                           c->grid.n[0] == c->th.nx && c->grid.n[1] == c->th.ny && c->grid.n[2] == c->th.nz && c->plan_foci == c->th_src_foci;
        if (!whole) return fail(c, OLX_ESTATE, "olx_thermal_run: the resident result holds no whole-grid intensity of %d foci on the thermal grid", c->th_src_foci);
        inten = c->d_inten;
    }
    if (c->th_max_focus >= c->th_src_foci) return fail(c, OLX_EINVAL, "olx_thermal_run: the schedule names focus %d, the source has %d", c->th_max_focus, c->th_src_foci);
    HIPCHK(c, hipSetDevice(c->device));
    if (c->th_src_resident && !c->th_src_pii) {      // (a deriving plan forms its intensity volumes here, once every check of this call has passed)
        int rc = materialize_intensity(c); if (rc) return rc;
        inten = c->d_inten;
    }
    const size_t vox = (size_t)c->th.vox;
    if (first_step == 0) {
        for (float* p : {(float*)c->d_th_T[0], (float*)c->d_th_max, (float*)c->d_th_cem}) HIPCHK(c, hipMemsetAsync(p, 0, sizeof(float) * vox, c->stream));
        c->th_cur = 0;
    }
    ThermalStep S{};
    S.dt = (float)dt; S.dt_min = (float)(dt / 60.0); S.tb43 = (float)(baseline - 43.0);
    S.npts = c->th_npts; S.n_foci = c->th_src_foci;
    for (int n = first_step; n < first_step + n_steps; ++n) olx_thermal_step(c, inten, n, S);
    if (n_steps > 0) olx_thermal_trace_last(c, first_step + n_steps - 1);
    HIPCHK(c, hipGetLastError());
    c->th_next = first_step + n_steps;
    return OLX_OK;
}

int olx_thermal_fetch(olx_ctx* c, float* rise_max, float* cem43, float* traces) {
    if (!c) return OLX_EINVAL;
    if (!c->th_planned || c->th_next < 0) return fail(c, OLX_ESTATE, "olx_thermal_fetch: nothing run");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
#ifdef OLX_DEBUG_BOUNDS
    { int rc_ = report_bounds(c); if (rc_) return rc_; }
#endif
    const size_t vox = (size_t)c->th.vox;
    int rc = OLX_OK;
    if (rise_max) rc = fetch_to_host(c, rise_max, c->d_th_max, sizeof(float) * vox);
    if (!rc && cem43) rc = fetch_to_host(c, cem43, c->d_th_cem, sizeof(float) * vox);
    if (!rc && traces && c->th_npts > 0) rc = fetch_to_host(c, traces, c->d_th_trace, sizeof(float) * (size_t)c->th_next * c->th_npts);
    return rc;
}

}  // extern "C"

// ---- full-wave model (kernel 5, k_fullwave.hip) ------------------------------------------------------------------------------------
extern "C" {

int olx_fullwave_plan(olx_ctx* c, const olx_grid* g, const float* sound_speed, const float* density, const float* absorption, double sound_speed0,
                      double density0, double absorption0, double c_ref, int pml_size, double pml_alpha, double dt, double* dt_max_out) {
    if (!c) return OLX_EINVAL;
    if (!g) return fail(c, OLX_EINVAL, "olx_fullwave_plan: null grid");
    double ih2 = 0;
    for (int a = 0; a < 3; ++a) {
        if (g->n[a] < 1 || !(g->spacing[a] > 0) || !std::isfinite(g->spacing[a])) return fail(c, OLX_EINVAL, "olx_fullwave_plan: bad grid axis %d", a);
        ih2 += 1.0 / (g->spacing[a] * g->spacing[a]);
    }
    const long long voxll = (long long)g->n[0] * g->n[1] * g->n[2];
    if (voxll >= (1ll << 31)) return fail(c, OLX_EINVAL, "olx_fullwave_plan: grid of %lld voxels is too large (< 2^31)", voxll);
    if (pml_size < 0 || !(pml_alpha >= 0) || !std::isfinite(pml_alpha)) return fail(c, OLX_EINVAL, "olx_fullwave_plan: pml_size must be >= 0, pml_alpha finite and >= 0");
    for (int a = 0; a < 3; ++a)
        if (2 * pml_size >= g->n[a]) return fail(c, OLX_EINVAL, "olx_fullwave_plan: axis %d of %d voxels holds no interior between two layers of %d", a, g->n[a], pml_size);
    if (!(c_ref > 0) || !std::isfinite(c_ref)) return fail(c, OLX_EINVAL, "olx_fullwave_plan: c_ref must be finite and > 0");
    if ((!sound_speed && !(sound_speed0 > 0 && std::isfinite(sound_speed0))) || (!density && !(density0 > 0 && std::isfinite(density0))) ||
        (!absorption && !(absorption0 >= 0 && std::isfinite(absorption0))))
        return fail(c, OLX_EINVAL, "olx_fullwave_plan: the scalars of NULL volumes must be finite and > 0 (absorption >= 0)");
    if (!(dt > 0) || !std::isfinite(dt)) return fail(c, OLX_EINVAL, "olx_fullwave_plan: dt must be finite and > 0");
    const size_t vox = (size_t)voxll;
    double c_max = sound_speed ? 0.0 : sound_speed0;
    for (size_t o = 0; o < vox; ++o) {
        if (sound_speed) {
            if (!(sound_speed[o] > 0.f) || !std::isfinite(sound_speed[o])) return fail(c, OLX_EINVAL, "olx_fullwave_plan: sound speed must be finite and > 0");
            c_max = std::max(c_max, (double)sound_speed[o]);
        }
        if (density && (!(density[o] > 0.f) || !std::isfinite(density[o]))) return fail(c, OLX_EINVAL, "olx_fullwave_plan: density must be finite and > 0");
        if (absorption && (!(absorption[o] >= 0.f) || !std::isfinite(absorption[o]))) return fail(c, OLX_EINVAL, "olx_fullwave_plan: absorption must be finite and >= 0");
    }
    const double dt_max = 6.0 / (7.0 * c_max * std::sqrt(ih2));
    if (dt_max_out) *dt_max_out = dt_max;
    if (dt > dt_max * (1.0 + 1e-6)) return fail(c, OLX_EINVAL, "olx_fullwave_plan: dt = %g s is above the stability bound %g s", dt, dt_max);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->fw_planned = false; c->fw_sourced = false; c->fw_next = -1;
    FullwaveParams& P = c->fw;
    P = FullwaveParams{};
    P.nx = g->n[0]; P.ny = g->n[1]; P.nz = g->n[2]; P.vox = voxll;
    P.ihx = (float)(1.0 / g->spacing[0]); P.ihy = (float)(1.0 / g->spacing[1]); P.ihz = (float)(1.0 / g->spacing[2]);
    P.dthx = (float)(dt / g->spacing[0]); P.dthy = (float)(dt / g->spacing[1]); P.dthz = (float)(dt / g->spacing[2]);
    P.dt = (float)dt;
    P.c0 = (float)sound_speed0; P.rho0 = (float)density0; P.alpha0 = (float)absorption0;
    c->fw_uniform = !sound_speed && !density && !absorption;
    c->fw_dt = dt; c->fw_dt_max = dt_max; c->fw_elem = false; c->fw_drive_mode = 0;
    c->fw_layers = 0; c->fw_pml = pml_size; c->fw_pml_alpha = pml_alpha; c->fw_c_ref = c_ref;   // every plan returns to the sponge (olx_fullwave_layers)
    for (int a = 0; a < 3; ++a) { c->fw_h[a] = g->spacing[a]; c->fw_origin[a] = g->origin[a]; }
    for (DevBuf<float>* b : {&c->d_fw_p, &c->d_fw_v[0], &c->d_fw_v[1], &c->d_fw_v[2], &c->d_fw_pmax, &c->d_fw_pmin}) { int rc = b->reserve(c, vox); if (rc) return rc; }
    // the layers' decay per step: d_a[i] = exp(-pml_alpha (c_ref / h_a) (depth / pml_size)^4 dt), depth = voxels into the layer (0 inside)
    const int ntab = P.nx + P.ny + P.nz;
    std::vector<float> tab(ntab);
    for (int a = 0, at = 0; a < 3; at += g->n[a], ++a)
        for (int i = 0; i < g->n[a]; ++i) {
            const int depth = i < pml_size ? pml_size - i : i >= g->n[a] - pml_size ? i - (g->n[a] - pml_size) + 1 : 0;
            const double x = pml_size > 0 ? (double)depth / pml_size : 0.0;
            tab[at + i] = (float)std::exp(-pml_alpha * (c_ref / g->spacing[a]) * x * x * x * x * dt);
        }
    { int rc = c->d_fw_dtab.reserve(c, ntab); if (rc) return rc; }
    HIPCHK(c, hipMemcpy(c->d_fw_dtab, tab.data(), sizeof(float) * ntab, hipMemcpyHostToDevice));
    if (c->fw_uniform) {
        P.bx0 = (float)(dt / (density0 * g->spacing[0])); P.by0 = (float)(dt / (density0 * g->spacing[1])); P.bz0 = (float)(dt / (density0 * g->spacing[2]));
        P.kp0 = (float)(dt * density0 * sound_speed0 * sound_speed0);
        P.ga0 = (float)std::exp(-2.0 * absorption0 * sound_speed0 * dt);
    } else {
        // the volumes go up once, the pack kernel forms the coefficients, the volumes are freed again
        DevScratch scr;
        const float* src[3] = {sound_speed, density, absorption};
        size_t nvol = 0;
        for (const float* p : src) nvol += p ? 1 : 0;
        HIPCHK(c, hipMalloc(&scr.p, sizeof(float) * vox * std::max(nvol, (size_t)1)));
        const float* dv[3] = {nullptr, nullptr, nullptr};
        size_t at = 0;
        for (int q = 0; q < 3; ++q) {
            if (!src[q]) continue;
            float* d = scr.at<float>(sizeof(float) * vox * at++);
            HIPCHK(c, hipMemcpy(d, src[q], sizeof(float) * vox, hipMemcpyHostToDevice));
            dv[q] = d;
        }
        for (DevBuf<float>& b : c->d_fw_coef) { int rc = b.reserve(c, vox); if (rc) return rc; }
        olx_fullwave_pack(c, dv[0], dv[1], dv[2]);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    c->fw_planned = true;
    c->fw_steps = 0; c->fw_npts = 0; c->fw_entries = 0;
    return OLX_OK;
}

int olx_fullwave_layers(olx_ctx* c, int model) {
    if (!c) return OLX_EINVAL;
    if (!c->fw_planned) return fail(c, OLX_ESTATE, "olx_fullwave_layers: no full-wave plan");
    if (model != 0 && model != 1) return fail(c, OLX_EINVAL, "olx_fullwave_layers: model must be 0 (sponge) or 1 (split layers), got %d", model);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // as a source call: the sources, the lock-in and the run state go
    c->fw_sourced = false; c->fw_next = -1; c->fw_elem = false; c->fw_drive_mode = 0;
    c->fw_lock = false; c->fw_lock_vol = false; c->fw_lock_nrec = 0; c->fw_lock_entries = 0;
    c->fw_steps = 0; c->fw_npts = 0; c->fw_entries = 0;
    c->fw_layers = 0;
    if (model == 0) return OLX_OK;
    // r_a[i] = exp(-sigma_a(d_c(i)) dt / 2), s_a[i] = exp(-sigma_a(d_f(i)) dt / 2), sigma_a(d) = pml_alpha (c_ref / h_a) (d / pml_size)^4: the depth of the
    // voxel's centre and of its + face, in voxels; formed in fp64 and rounded once
    const FullwaveParams& P = c->fw;
    const int ng[3] = {P.nx, P.ny, P.nz}, ntab = P.nx + P.ny + P.nz, pml = c->fw_pml;
    std::vector<float> rt(ntab), st(ntab);
    for (int a = 0, at = 0; a < 3; at += ng[a], ++a)
        for (int i = 0; i < ng[a]; ++i) {
            const double last = (double)(ng[a] - 1 - pml);
            const double dc = std::max(std::max((double)pml - i, i - last), 0.0), df = std::max(std::max((double)pml - (i + 0.5), (i + 0.5) - last), 0.0);
            const double xc = pml > 0 ? dc / pml : 0.0, xf = pml > 0 ? df / pml : 0.0;
            const double k = c->fw_pml_alpha * (c->fw_c_ref / c->fw_h[a]);
            rt[at + i] = (float)std::exp(-(k * (xc * xc * xc * xc)) * c->fw_dt / 2);
            st[at + i] = (float)std::exp(-(k * (xf * xf * xf * xf)) * c->fw_dt / 2);
        }
    int rc = c->d_fw_rtab.reserve(c, ntab);
    if (!rc) rc = c->d_fw_stab.reserve(c, ntab);
    for (DevBuf<float>& b : c->d_fw_pc) if (!rc) rc = b.reserve(c, (size_t)P.vox);
    if (rc) return rc;
    HIPCHK(c, hipMemcpy(c->d_fw_rtab, rt.data(), sizeof(float) * ntab, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_fw_stab, st.data(), sizeof(float) * ntab, hipMemcpyHostToDevice));
    c->fw_layers = 1;
    return OLX_OK;
}

// the split model takes sources on interior voxels only: true when linear voxel `at` lies in a layer
static bool fw_in_layer(const olx_ctx* c, long long at) {
    const FullwaveParams& P = c->fw;
    const int pml = c->fw_pml, k = (int)(at % P.nz), j = (int)((at / P.nz) % P.ny), i = (int)(at / ((long long)P.nz * P.ny));
    return i < pml || i >= P.nx - pml || j < pml || j >= P.ny - pml || k < pml || k >= P.nz - pml;
}

int olx_fullwave_sources(olx_ctx* c, int n_entries, const long long* voxels, const double* amplitude, const double* tau_s, double freq, double cycles,
                         double ramp_cycles, int n_steps, int n_points, const long long* points) {
    if (!c) return OLX_EINVAL;
    if (!c->fw_planned) return fail(c, OLX_ESTATE, "olx_fullwave_sources: no full-wave plan");
    if (n_entries < 0 || (n_entries > 0 && (!voxels || !amplitude || !tau_s))) return fail(c, OLX_EINVAL, "olx_fullwave_sources: n_entries < 0 or null table");
    if (!(freq > 0) || !std::isfinite(freq) || !(cycles > 0) || !std::isfinite(cycles) || !(ramp_cycles >= 0) || !std::isfinite(ramp_cycles))
        return fail(c, OLX_EINVAL, "olx_fullwave_sources: freq and cycles must be finite and > 0, ramp_cycles finite and >= 0");
    if (n_steps < 1 || n_points < 0 || (n_points > 0 && !points)) return fail(c, OLX_EINVAL, "olx_fullwave_sources: n_steps < 1 or bad points");
    for (int e = 0; e < n_entries; ++e) {
        if (voxels[e] < 0 || voxels[e] >= c->fw.vox) return fail(c, OLX_EINVAL, "olx_fullwave_sources: entry %d: voxel %lld outside the grid of %lld voxels", e, voxels[e], c->fw.vox);
        if (c->fw_layers == 1 && fw_in_layer(c, voxels[e])) return fail(c, OLX_EINVAL, "olx_fullwave_sources: entry %d: voxel %lld lies in a layer (the split layers take sources on interior voxels only)", e, voxels[e]);
        if (!std::isfinite(amplitude[e]) || !std::isfinite(tau_s[e])) return fail(c, OLX_EINVAL, "olx_fullwave_sources: entry %d: amplitude and delay must be finite", e);
    }
    for (int p = 0; p < n_points; ++p)
        if (points[p] < 0 || points[p] >= c->fw.vox) return fail(c, OLX_EINVAL, "olx_fullwave_sources: trace point %d outside the grid", p);
    if ((double)n_steps * n_points > 268435456.0) return fail(c, OLX_EINVAL, "olx_fullwave_sources: %g trace samples are too many (trace fewer points)", (double)n_steps * n_points);
    // CSR by voxel: a stable sort keeps the entries of one voxel in table order
    std::vector<int> order(n_entries);
    for (int e = 0; e < n_entries; ++e) order[e] = e;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return voxels[a] < voxels[b]; });
    std::vector<long long> svox; std::vector<int> srow; std::vector<double> samp(n_entries), stau(n_entries);
    for (int q = 0; q < n_entries; ++q) {
        const int e = order[q];
        if (q == 0 || voxels[e] != svox.back()) { svox.push_back(voxels[e]); srow.push_back(q); }
        samp[q] = amplitude[e]; stau[q] = tau_s[e];
    }
    srow.push_back(n_entries);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->fw_sourced = false; c->fw_next = -1;
    c->fw_lock = false; c->fw_lock_vol = false; c->fw_lock_nrec = 0; c->fw_lock_entries = 0;   // a new source table runs without a lock-in until olx_fullwave_lockin asks for one
    int rc = c->d_fw_svox.reserve(c, svox.size());
    if (!rc) rc = c->d_fw_srow.reserve(c, srow.size());
    if (!rc) rc = c->d_fw_samp.reserve(c, n_entries);
    if (!rc) rc = c->d_fw_stau.reserve(c, n_entries);
    if (!rc) rc = c->d_fw_pts.reserve(c, n_points);
    if (!rc) rc = c->d_fw_trace.reserve(c, (size_t)n_steps * n_points);
    if (rc) return rc;
    if (n_entries > 0) {
        HIPCHK(c, hipMemcpy(c->d_fw_svox, svox.data(), sizeof(long long) * svox.size(), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(c->d_fw_samp, samp.data(), sizeof(double) * n_entries, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(c->d_fw_stau, stau.data(), sizeof(double) * n_entries, hipMemcpyHostToDevice));
    }
    HIPCHK(c, hipMemcpy(c->d_fw_srow, srow.data(), sizeof(int) * srow.size(), hipMemcpyHostToDevice));
    if (n_points > 0) HIPCHK(c, hipMemcpy(c->d_fw_pts, points, sizeof(long long) * n_points, hipMemcpyHostToDevice));
    FullwaveSource& S = c->fw_src;
    S = FullwaveSource{};
    S.freq = freq; S.T = cycles / freq; S.Tr = ramp_cycles / freq; S.dt = c->fw_dt; S.n_vox = (int)svox.size();
    c->fw_entries = n_entries; c->fw_steps = n_steps; c->fw_npts = n_points; c->fw_elem = false; c->fw_drive_mode = 0;
    c->fw_sourced = true;
    return OLX_OK;
}

int olx_fullwave_sources_elements(olx_ctx* c, int n_entries, const long long* voxels, const int* elements, const double* amplitude, int n_el, const double* A,
                                  const double* tau_s, double freq, double cycles, double ramp_cycles, int n_steps, int n_points, const long long* points) {
    if (!c) return OLX_EINVAL;
    if (!c->fw_planned) return fail(c, OLX_ESTATE, "olx_fullwave_sources_elements: no full-wave plan");
    if (n_entries < 0 || (n_entries > 0 && (!voxels || !elements || !amplitude))) return fail(c, OLX_EINVAL, "olx_fullwave_sources_elements: n_entries < 0 or null table");
    if (n_el < 1 || !A || !tau_s) return fail(c, OLX_EINVAL, "olx_fullwave_sources_elements: n_el < 1 or null A / tau");
    if (!(freq > 0) || !std::isfinite(freq) || !(cycles > 0) || !std::isfinite(cycles) || !(ramp_cycles >= 0) || !std::isfinite(ramp_cycles))
        return fail(c, OLX_EINVAL, "olx_fullwave_sources_elements: freq and cycles must be finite and > 0, ramp_cycles finite and >= 0");
    if (n_steps < 1 || n_points < 0 || (n_points > 0 && !points)) return fail(c, OLX_EINVAL, "olx_fullwave_sources_elements: n_steps < 1 or bad points");
    for (int e = 0; e < n_el; ++e)
        if (!std::isfinite(A[e]) || !std::isfinite(tau_s[e])) return fail(c, OLX_EINVAL, "olx_fullwave_sources_elements: element %d: A and delay must be finite", e);
    for (int q = 0; q < n_entries; ++q) {
        if (voxels[q] < 0 || voxels[q] >= c->fw.vox) return fail(c, OLX_EINVAL, "olx_fullwave_sources_elements: entry %d: voxel %lld outside the grid of %lld voxels", q, voxels[q], c->fw.vox);
        if (c->fw_layers == 1 && fw_in_layer(c, voxels[q])) return fail(c, OLX_EINVAL, "olx_fullwave_sources_elements: entry %d: voxel %lld lies in a layer (the split layers take sources on interior voxels only)", q, voxels[q]);
        if (elements[q] < 0 || elements[q] >= n_el) return fail(c, OLX_EINVAL, "olx_fullwave_sources_elements: entry %d: element %d outside [0, %d)", q, elements[q], n_el);
        if (!std::isfinite(amplitude[q])) return fail(c, OLX_EINVAL, "olx_fullwave_sources_elements: entry %d: amplitude must be finite", q);
    }
    for (int p = 0; p < n_points; ++p)
        if (points[p] < 0 || points[p] >= c->fw.vox) return fail(c, OLX_EINVAL, "olx_fullwave_sources_elements: trace point %d outside the grid", p);
    if ((double)n_steps * n_points > 268435456.0) return fail(c, OLX_EINVAL, "olx_fullwave_sources_elements: %g trace samples are too many (trace fewer points)", (double)n_steps * n_points);
    if ((double)n_steps * n_el * sizeof(double) > 268435456.0)
        return fail(c, OLX_EINVAL, "olx_fullwave_sources_elements: a drive table of %d steps x %d elements (%g bytes) is too large (2^28 bytes)", n_steps, n_el, (double)n_steps * n_el * sizeof(double));
    // CSR by voxel: a stable sort keeps the entries of one voxel in table order (ascending element for a table built element by element)
    std::vector<int> order(n_entries);
    for (int q = 0; q < n_entries; ++q) order[q] = q;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return voxels[a] < voxels[b]; });
    std::vector<long long> svox; std::vector<int> srow, sel(n_entries); std::vector<double> samp(n_entries);
    for (int q = 0; q < n_entries; ++q) {
        const int e = order[q];
        if (q == 0 || voxels[e] != svox.back()) { svox.push_back(voxels[e]); srow.push_back(q); }
        samp[q] = amplitude[e]; sel[q] = elements[e];
    }
    srow.push_back(n_entries);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->fw_sourced = false; c->fw_next = -1;
    c->fw_lock = false; c->fw_lock_vol = false; c->fw_lock_nrec = 0; c->fw_lock_entries = 0;
    int rc = c->d_fw_svox.reserve(c, svox.size());
    if (!rc) rc = c->d_fw_srow.reserve(c, srow.size());
    if (!rc) rc = c->d_fw_samp.reserve(c, n_entries);
    if (!rc) rc = c->d_fw_sel.reserve(c, n_entries);
    if (!rc) rc = c->d_fw_dA.reserve(c, n_el);
    if (!rc) rc = c->d_fw_dtau.reserve(c, n_el);
    if (!rc) rc = c->d_fw_drive.reserve(c, (size_t)n_steps * n_el);
    if (!rc) rc = c->d_fw_pts.reserve(c, n_points);
    if (!rc) rc = c->d_fw_trace.reserve(c, (size_t)n_steps * n_points);
    if (rc) return rc;
    if (n_entries > 0) {
        HIPCHK(c, hipMemcpy(c->d_fw_svox, svox.data(), sizeof(long long) * svox.size(), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(c->d_fw_samp, samp.data(), sizeof(double) * n_entries, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(c->d_fw_sel, sel.data(), sizeof(int) * n_entries, hipMemcpyHostToDevice));
    }
    HIPCHK(c, hipMemcpy(c->d_fw_srow, srow.data(), sizeof(int) * srow.size(), hipMemcpyHostToDevice));
    if (n_points > 0) HIPCHK(c, hipMemcpy(c->d_fw_pts, points, sizeof(long long) * n_points, hipMemcpyHostToDevice));
    FullwaveSource& S = c->fw_src;
    S = FullwaveSource{};
    S.freq = freq; S.T = cycles / freq; S.Tr = ramp_cycles / freq; S.dt = c->fw_dt; S.n_vox = (int)svox.size();
    c->fw_entries = n_entries; c->fw_steps = n_steps; c->fw_npts = n_points; c->fw_elem = true; c->fw_nel = n_el; c->fw_drive_mode = 0;   // a source call returns to the bare drive
    c->fw_sourced = true;
    return olx_fullwave_drive(c, A, tau_s);
}

int olx_fullwave_drive(olx_ctx* c, const double* A, const double* tau_s) {
    if (!c) return OLX_EINVAL;
    if (!c->fw_planned || !c->fw_sourced || !c->fw_elem) return fail(c, OLX_ESTATE, "olx_fullwave_drive: needs olx_fullwave_sources_elements as the last source call");
    if (c->fw_drive_mode == 2) return fail(c, OLX_ESTATE, "olx_fullwave_drive: the drive table is a sampled one (olx_fullwave_drive_table); A and tau mean nothing to it until the next source call");
    if (!A || !tau_s) return fail(c, OLX_EINVAL, "olx_fullwave_drive: null A / tau");
    for (int e = 0; e < c->fw_nel; ++e)
        if (!std::isfinite(A[e]) || !std::isfinite(tau_s[e])) return fail(c, OLX_EINVAL, "olx_fullwave_drive: element %d: A and delay must be finite", e);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->fw_next = -1;                            // the run starts again, without a lock-in until olx_fullwave_lockin asks for one
    c->fw_lock = false; c->fw_lock_vol = false; c->fw_lock_nrec = 0; c->fw_lock_entries = 0;
    HIPCHK(c, hipMemcpy(c->d_fw_dA, A, sizeof(double) * c->fw_nel, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_fw_dtau, tau_s, sizeof(double) * c->fw_nel, hipMemcpyHostToDevice));
    olx_fullwave_drive_fill(c);
    HIPCHK(c, hipGetLastError());
    return OLX_OK;
}

// the run starts again, without a lock-in until olx_fullwave_lockin asks for one (the reset of olx_fullwave_drive)
static void fw_drive_reset(olx_ctx* c) {
    c->fw_next = -1;
    c->fw_lock = false; c->fw_lock_vol = false; c->fw_lock_nrec = 0; c->fw_lock_entries = 0;
}

int olx_fullwave_drive_response(olx_ctx* c, int n_classes, const int32_t* class_of_element, const int32_t* row, const double* taps) {
    if (!c) return OLX_EINVAL;
    if (!c->fw_planned || !c->fw_sourced || !c->fw_elem) return fail(c, OLX_ESTATE, "olx_fullwave_drive_response: needs olx_fullwave_sources_elements as the last source call");
    if (c->fw_drive_mode == 2) return fail(c, OLX_ESTATE, "olx_fullwave_drive_response: the drive table is a sampled one (olx_fullwave_drive_table) until the next source call");
    const int n_el = c->fw_nel;
    int m_max = 0;
    if (n_classes != 0) {
        if (n_classes < 0 || n_classes > n_el)
            return fail(c, OLX_EINVAL, "olx_fullwave_drive_response: %d classes for %d elements (0 returns to the bare drive, at most one class per element)", n_classes, n_el);
        if (!class_of_element || !row || !taps) return fail(c, OLX_EINVAL, "olx_fullwave_drive_response: null pointer");
        if (row[0] != 0) return fail(c, OLX_EINVAL, "olx_fullwave_drive_response: the row table must start at 0, got %d", (int)row[0]);
        for (int r = 0; r < n_classes; ++r) {
            if (row[r + 1] <= row[r]) return fail(c, OLX_EINVAL, "olx_fullwave_drive_response: the row table must be strictly increasing (class %d has no taps)", r);
            if (row[r + 1] - row[r] > OLX_PULSE_RESPONSE_MAX_TAPS)
                return fail(c, OLX_EINVAL, "olx_fullwave_drive_response: class %d has %d taps, at most OLX_PULSE_RESPONSE_MAX_TAPS = %d", r, (int)(row[r + 1] - row[r]),
                            OLX_PULSE_RESPONSE_MAX_TAPS);
            m_max = std::max(m_max, (int)(row[r + 1] - row[r]));
        }
        for (int e = 0; e < n_el; ++e)
            if (class_of_element[e] < 0 || class_of_element[e] >= n_classes)
                return fail(c, OLX_EINVAL, "olx_fullwave_drive_response: element %d: class %d outside 0 .. %d", e, (int)class_of_element[e], n_classes - 1);
        for (int g = 0; g < row[n_classes]; ++g)
            if (!std::isfinite(taps[g])) return fail(c, OLX_EINVAL, "olx_fullwave_drive_response: tap %d is not finite", g);
        const double ext_bytes = ((double)c->fw_steps + (m_max - 1)) * n_el * sizeof(double);
        if (ext_bytes > 268435456.0)
            return fail(c, OLX_EINVAL, "olx_fullwave_drive_response: an extended drive table of (%d + %d) steps x %d elements (%g bytes) is too large (2^28 bytes)",
                        c->fw_steps, m_max - 1, n_el, ext_bytes);
    }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // the run and the lock-in are reset only once the tables stand on the device: a call that fails before leaves the drive table, the run and the
    // lock-in as they were
    if (n_classes == 0) {
        c->fw_drive_mode = 0;
    } else {
        static_assert(sizeof(int) == sizeof(int32_t), "the class and row tables go up as they are");
        const int n_taps = row[n_classes];
        int rc = c->d_fw_gcls.reserve(c, n_el);
        if (!rc) rc = c->d_fw_grow.reserve(c, (size_t)n_classes + 1);
        if (!rc) rc = c->d_fw_gtaps.reserve(c, n_taps);
        if (!rc) rc = c->d_fw_dext.reserve(c, ((size_t)c->fw_steps + (m_max - 1)) * n_el);
        if (rc) return rc;
        HIPCHK(c, hipMemcpy(c->d_fw_gcls, class_of_element, sizeof(int) * n_el, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(c->d_fw_grow, row, sizeof(int) * ((size_t)n_classes + 1), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(c->d_fw_gtaps, taps, sizeof(double) * n_taps, hipMemcpyHostToDevice));
        c->fw_drive_mode = 1; c->fw_resp_classes = n_classes; c->fw_resp_ntaps = n_taps; c->fw_resp_mmax = m_max;
    }
    fw_drive_reset(c);
    olx_fullwave_drive_fill(c);
    HIPCHK(c, hipGetLastError());
    return OLX_OK;
}

int olx_fullwave_drive_table(olx_ctx* c, const double* table) {
    if (!c) return OLX_EINVAL;
    if (!c->fw_planned || !c->fw_sourced || !c->fw_elem) return fail(c, OLX_ESTATE, "olx_fullwave_drive_table: needs olx_fullwave_sources_elements as the last source call");
    if (!table) return fail(c, OLX_EINVAL, "olx_fullwave_drive_table: null table");
    const size_t total = (size_t)c->fw_steps * c->fw_nel;
    for (size_t g = 0; g < total; ++g)
        if (!std::isfinite(table[g]))
            return fail(c, OLX_EINVAL, "olx_fullwave_drive_table: step %lld, element %d: the drive must be finite", (long long)(g / c->fw_nel), (int)(g % c->fw_nel));
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    fw_drive_reset(c);      // before the copy, on purpose: a copy that fails leaves a table that is neither the old nor the new one, and no run may continue over it
    HIPCHK(c, hipMemcpy(c->d_fw_drive, table, sizeof(double) * total, hipMemcpyHostToDevice));
    c->fw_drive_mode = 2;
    return OLX_OK;
}

int olx_fullwave_fetch_drive(olx_ctx* c, double* table) {
    if (!c) return OLX_EINVAL;
    if (!c->fw_planned || !c->fw_sourced || !c->fw_elem) return fail(c, OLX_ESTATE, "olx_fullwave_fetch_drive: needs olx_fullwave_sources_elements as the last source call");
    if (!table) return fail(c, OLX_EINVAL, "olx_fullwave_fetch_drive: null table");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
#ifdef OLX_DEBUG_BOUNDS
    { int rc_ = report_bounds(c); if (rc_) return rc_; }
#endif
    HIPCHK(c, hipMemcpy(table, c->d_fw_drive, sizeof(double) * (size_t)c->fw_steps * c->fw_nel, hipMemcpyDeviceToHost));
    return OLX_OK;
}

int olx_fullwave_apertures(olx_ctx* c, int n_el, const double* centre, const double* u_axis, const double* v_axis, const double* size, const int* n_w,
                           const int* n_l, long long capacity, int* row, long long* voxels, double* weights, long long* n_needed) {
    if (!c) return OLX_EINVAL;
    if (!c->fw_planned) return fail(c, OLX_ESTATE, "olx_fullwave_apertures: no full-wave plan");
    if (n_el < 1 || !centre || !u_axis || !v_axis || !size || !n_w || !n_l || !row) return fail(c, OLX_EINVAL, "olx_fullwave_apertures: n_el < 1 or null argument");
    if (capacity < 0 || (capacity > 0 && (!voxels || !weights))) return fail(c, OLX_EINVAL, "olx_fullwave_apertures: capacity < 0 or null output");
    const FullwaveParams& P = c->fw;
    const int ng[3] = {P.nx, P.ny, P.nz};
    std::vector<FullwaveAperture> ap(n_el);
    long long total = 0, max_box = 0;
    for (int e = 0; e < n_el; ++e) {
        FullwaveAperture& E = ap[e];
        for (int a = 0; a < 3; ++a) { E.c[a] = centre[3 * e + a]; E.u[a] = u_axis[3 * e + a]; E.v[a] = v_axis[3 * e + a]; }
        E.w = size[2 * e]; E.l = size[2 * e + 1]; E.nw = n_w[e]; E.nl = n_l[e];
        bool finite = std::isfinite(E.w) && std::isfinite(E.l);
        for (int a = 0; a < 3; ++a) finite = finite && std::isfinite(E.c[a]) && std::isfinite(E.u[a]) && std::isfinite(E.v[a]);
        if (!finite) return fail(c, OLX_EINVAL, "olx_fullwave_apertures: element %d: centre, axes and size must be finite", e);
        if (E.w < 0 || E.l < 0) return fail(c, OLX_EINVAL, "olx_fullwave_apertures: element %d: size (%g, %g) m must be >= 0", e, E.w, E.l);
        if (E.nw < 1 || E.nl < 1) return fail(c, OLX_EINVAL, "olx_fullwave_apertures: element %d: n_w = %d, n_l = %d must be >= 1", e, E.nw, E.nl);
        if ((long long)E.nw * E.nl > 65536) return fail(c, OLX_EINVAL, "olx_fullwave_apertures: element %d: %lld points are too many (65536)", e, (long long)E.nw * E.nl);
        // the extreme points bound every point's coordinates (each operation is monotone): their weighted voxels decide the refusal; the
        // index box is that of the rectangle's four corners, floor(min) .. floor(max) + 1, clipped to the grid
        long long box = 1;
        for (int a = 0; a < 3; ++a) {
            double qlo = 0, qhi = 0, blo = 0, bhi = 0;
            for (int t = 0; t < 4; ++t) {
                const double q = fw_aperture_q(E, fw_aperture_s(t & 1 ? E.nw - 1 : 0, E.nw), fw_aperture_s(t & 2 ? E.nl - 1 : 0, E.nl), a, c->fw_origin[a], c->fw_h[a]);
                const double b = fw_aperture_q(E, t & 1 ? 0.5 : -0.5, t & 2 ? 0.5 : -0.5, a, c->fw_origin[a], c->fw_h[a]);
                if (t == 0 || q < qlo) qlo = q;
                if (t == 0 || q > qhi) qhi = q;
                if (t == 0 || b < blo) blo = b;
                if (t == 0 || b > bhi) bhi = b;
            }
            if (qlo < 0 || std::ceil(qhi) > ng[a] - 1)
                return fail(c, OLX_EINVAL, "olx_fullwave_apertures: element %d does not lie inside the grid (axis %d: its points span voxels %g .. %g of %d)", e, a, qlo, qhi, ng[a]);
            const int lo = (int)std::max(0.0, std::floor(std::min(blo, qlo))), hi = (int)std::min((double)(ng[a] - 1), std::floor(std::max(bhi, qhi)) + 1.0);
            E.lo[a] = lo; E.dim[a] = hi - lo + 1;
            box *= E.dim[a];
        }
        E.off = total;
        total += box; max_box = std::max(max_box, box);
    }
    if (max_box > 65535ll * 256 || (double)total * sizeof(double) > 268435456.0)
        return fail(c, OLX_EINVAL, "olx_fullwave_apertures: index boxes of %lld voxels (largest %lld) are too large", total, max_box);
    HIPCHK(c, hipSetDevice(c->device));
    int rc = c->d_fw_ap.reserve(c, n_el);
    if (!rc) rc = c->d_fw_apw.reserve(c, (size_t)total);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->d_fw_ap, ap.data(), sizeof(FullwaveAperture) * n_el, hipMemcpyHostToDevice, c->stream));
    olx_fullwave_aperture_weights(c, n_el, max_box, total);
    HIPCHK(c, hipGetLastError());
    std::vector<double> dense((size_t)total);
    HIPCHK(c, hipMemcpyAsync(dense.data(), c->d_fw_apw, sizeof(double) * (size_t)total, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
#ifdef OLX_DEBUG_BOUNDS
    { int rc_ = report_bounds(c); if (rc_) return rc_; }
#endif
    // per-element CSR of the weights that are not 0, in the box's C order: ascending linear voxel inside a row
    long long n = 0;
    for (int e = 0; e < n_el; ++e) {
        if (n > 2147483647ll) break;
        row[e] = (int)n;
        const FullwaveAperture& E = ap[e];
        long long t = E.off;
        for (int i = 0; i < E.dim[0]; ++i)
            for (int j = 0; j < E.dim[1]; ++j)
                for (int k = 0; k < E.dim[2]; ++k, ++t) {
                    if (dense[(size_t)t] == 0.0) continue;
                    if (n < capacity) { voxels[n] = ((long long)(E.lo[0] + i) * P.ny + (E.lo[1] + j)) * P.nz + (E.lo[2] + k); weights[n] = dense[(size_t)t]; }
                    ++n;
                }
    }
    if (n > 2147483647ll) return fail(c, OLX_EINVAL, "olx_fullwave_apertures: more than 2^31 - 1 entries");
    row[n_el] = (int)n;
    if (n_needed) *n_needed = n;
    return OLX_OK;
}

int olx_fullwave_run(olx_ctx* c, int first_step, int n_steps, int accumulate_psq) {
    if (!c) return OLX_EINVAL;
    if (!c->fw_planned || !c->fw_sourced) return fail(c, OLX_ESTATE, "olx_fullwave_run: needs olx_fullwave_plan and olx_fullwave_sources first");
    if (n_steps < 0 || first_step < 0 || first_step + n_steps > c->fw_steps) return fail(c, OLX_EINVAL, "olx_fullwave_run: steps [%d, %d) outside the run of %d", first_step, first_step + n_steps, c->fw_steps);
    if (first_step > 0 && first_step != c->fw_next) return fail(c, OLX_ESTATE, "olx_fullwave_run: step %d does not continue the last run (next step %d)", first_step, c->fw_next);
    const bool pii = accumulate_psq != 0;
    if (first_step > 0 && pii != c->fw_pii) return fail(c, OLX_ESTATE, "olx_fullwave_run: a continued run keeps the accumulation of sum p^2 as the run began it");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t vox = (size_t)c->fw.vox;
    if (first_step == 0) {
        if (pii) { int rc = c->d_fw_psq.reserve(c, vox); if (rc) return rc; }
        for (float* p : {(float*)c->d_fw_p, (float*)c->d_fw_v[0], (float*)c->d_fw_v[1], (float*)c->d_fw_v[2], (float*)c->d_fw_pmax, (float*)c->d_fw_pmin})
            HIPCHK(c, hipMemsetAsync(p, 0, sizeof(float) * vox, c->stream));
        if (pii) HIPCHK(c, hipMemsetAsync(c->d_fw_psq, 0, sizeof(float) * vox, c->stream));
        if (c->fw_layers == 1)
            for (DevBuf<float>& b : c->d_fw_pc) HIPCHK(c, hipMemsetAsync(b, 0, sizeof(float) * vox, c->stream));
        c->fw_pii = pii;
        if (c->fw_lock && c->fw_lock_vol)
            for (float* p : {(float*)c->d_fw_lc, (float*)c->d_fw_ls}) HIPCHK(c, hipMemsetAsync(p, 0, sizeof(float) * vox, c->stream));
        if (c->fw_lock && c->fw_lock_nrec > 0)
            for (double* p : {(double*)c->d_fw_lrc, (double*)c->d_fw_lrs}) HIPCHK(c, hipMemsetAsync(p, 0, sizeof(double) * c->fw_lock_nrec, c->stream));
    }
    for (int n = first_step; n < first_step + n_steps; ++n) olx_fullwave_step(c, n, pii);
    HIPCHK(c, hipGetLastError());
    c->fw_next = first_step + n_steps;
    return OLX_OK;
}

int olx_fullwave_lockin(olx_ctx* c, double freq, int first_step, int n_steps, int volume, int n_receivers, const int* row, const long long* voxels,
                        const double* weights) {
    if (!c) return OLX_EINVAL;
    if (!c->fw_planned || !c->fw_sourced) return fail(c, OLX_ESTATE, "olx_fullwave_lockin: needs olx_fullwave_plan and olx_fullwave_sources first");
    if (!(freq > 0) || !std::isfinite(freq)) return fail(c, OLX_EINVAL, "olx_fullwave_lockin: freq must be finite and > 0");
    if (first_step < 0 || n_steps < 1 || (long long)first_step + n_steps > c->fw_steps)
        return fail(c, OLX_EINVAL, "olx_fullwave_lockin: window [%d, %lld) outside the run of %d steps", first_step, (long long)first_step + n_steps, c->fw_steps);
    if (n_receivers < 0 || (n_receivers > 0 && !row)) return fail(c, OLX_EINVAL, "olx_fullwave_lockin: n_receivers < 0 or null row table");
    if (!volume && n_receivers == 0) return fail(c, OLX_EINVAL, "olx_fullwave_lockin: neither the volume nor a receiver to record");
    int n_entries = 0;
    if (n_receivers > 0) {
        if (row[0] != 0) return fail(c, OLX_EINVAL, "olx_fullwave_lockin: row[0] must be 0");
        for (int r = 0; r < n_receivers; ++r)
            if (row[r + 1] < row[r]) return fail(c, OLX_EINVAL, "olx_fullwave_lockin: row table not monotone at receiver %d", r);
        n_entries = row[n_receivers];
        if (n_entries > 0 && (!voxels || !weights)) return fail(c, OLX_EINVAL, "olx_fullwave_lockin: null receiver table");
        for (int e = 0; e < n_entries; ++e) {
            if (voxels[e] < 0 || voxels[e] >= c->fw.vox) return fail(c, OLX_EINVAL, "olx_fullwave_lockin: entry %d: voxel %lld outside the grid of %lld voxels", e, voxels[e], c->fw.vox);
            if (!std::isfinite(weights[e])) return fail(c, OLX_EINVAL, "olx_fullwave_lockin: entry %d: weight must be finite", e);
        }
    }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->fw_lock = false; c->fw_next = -1;       // the records belong to the run that follows: olx_fullwave_run(first_step = 0)
    int rc = OLX_OK;
    if (volume) {
        rc = c->d_fw_lc.reserve(c, (size_t)c->fw.vox);
        if (!rc) rc = c->d_fw_ls.reserve(c, (size_t)c->fw.vox);
    }
    if (!rc && n_receivers > 0) {
        rc = c->d_fw_lrow.reserve(c, (size_t)n_receivers + 1);
        if (!rc) rc = c->d_fw_lvox.reserve(c, n_entries);
        if (!rc) rc = c->d_fw_lw.reserve(c, n_entries);
        if (!rc) rc = c->d_fw_lrc.reserve(c, n_receivers);
        if (!rc) rc = c->d_fw_lrs.reserve(c, n_receivers);
    }
    if (rc) return rc;
    if (n_receivers > 0) {
        HIPCHK(c, hipMemcpy(c->d_fw_lrow, row, sizeof(int) * ((size_t)n_receivers + 1), hipMemcpyHostToDevice));
        if (n_entries > 0) {
            HIPCHK(c, hipMemcpy(c->d_fw_lvox, voxels, sizeof(long long) * n_entries, hipMemcpyHostToDevice));
            HIPCHK(c, hipMemcpy(c->d_fw_lw, weights, sizeof(double) * n_entries, hipMemcpyHostToDevice));
        }
    }
    c->fw_lock_freq = freq; c->fw_lock_w0 = first_step; c->fw_lock_nw = n_steps;
    c->fw_lock_vol = volume != 0; c->fw_lock_nrec = n_receivers; c->fw_lock_entries = n_entries;
    c->fw_lock = true;
    return OLX_OK;
}

int olx_fullwave_fetch_lockin(olx_ctx* c, float* vol_cos, float* vol_sin, double* rec_cos, double* rec_sin) {
    if (!c) return OLX_EINVAL;
    if (!c->fw_planned || c->fw_next < 0) return fail(c, OLX_ESTATE, "olx_fullwave_fetch_lockin: nothing run");
    if (!c->fw_lock) return fail(c, OLX_ESTATE, "olx_fullwave_fetch_lockin: the run recorded no lock-in");
    if ((vol_cos || vol_sin) && !c->fw_lock_vol) return fail(c, OLX_ESTATE, "olx_fullwave_fetch_lockin: the run did not record the lock-in volume");
    if ((rec_cos || rec_sin) && c->fw_lock_nrec == 0) return fail(c, OLX_ESTATE, "olx_fullwave_fetch_lockin: the run did not record receivers");
    if (c->fw_next < c->fw_lock_w0 + c->fw_lock_nw)
        return fail(c, OLX_ESTATE, "olx_fullwave_fetch_lockin: the run stands at step %d, before the end of the window [%d, %d)", c->fw_next, c->fw_lock_w0, c->fw_lock_w0 + c->fw_lock_nw);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
#ifdef OLX_DEBUG_BOUNDS
    { int rc_ = report_bounds(c); if (rc_) return rc_; }
#endif
    const size_t vox = (size_t)c->fw.vox, nrec = (size_t)c->fw_lock_nrec;
    int rc = OLX_OK;
    if (vol_cos) rc = fetch_to_host(c, vol_cos, c->d_fw_lc, sizeof(float) * vox);
    if (!rc && vol_sin) rc = fetch_to_host(c, vol_sin, c->d_fw_ls, sizeof(float) * vox);
    if (!rc && rec_cos) rc = fetch_to_host(c, rec_cos, c->d_fw_lrc, sizeof(double) * nrec);
    if (!rc && rec_sin) rc = fetch_to_host(c, rec_sin, c->d_fw_lrs, sizeof(double) * nrec);
    return rc;
}

int olx_fullwave_fetch(olx_ctx* c, float* p_max, float* p_min, float* p_sq, float* traces) {
    if (!c) return OLX_EINVAL;
    if (!c->fw_planned || c->fw_next < 0) return fail(c, OLX_ESTATE, "olx_fullwave_fetch: nothing run");
    if (p_sq && !c->fw_pii) return fail(c, OLX_ESTATE, "olx_fullwave_fetch: the run did not accumulate sum p^2");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
#ifdef OLX_DEBUG_BOUNDS
    { int rc_ = report_bounds(c); if (rc_) return rc_; }
#endif
    const size_t vox = (size_t)c->fw.vox;
    int rc = OLX_OK;
    if (p_max) rc = fetch_to_host(c, p_max, c->d_fw_pmax, sizeof(float) * vox);
    if (!rc && p_min) rc = fetch_to_host(c, p_min, c->d_fw_pmin, sizeof(float) * vox);
    if (!rc && p_sq) rc = fetch_to_host(c, p_sq, c->d_fw_psq, sizeof(float) * vox);
    if (!rc && traces && c->fw_npts > 0 && c->fw_next > 0) rc = fetch_to_host(c, traces, c->d_fw_trace, sizeof(float) * (size_t)c->fw_next * c->fw_npts);
    return rc;
}

}  // extern "C"

// ---- eikonal travel times (kernel 6, k_eikonal.hip) ---------------------------------------------------------------------------------
extern "C" {

static constexpr int EK_CHECK = 8;     // the host reads the sweeps' flags after every EK_CHECK sweeps (once the launch box covers the grid)

int olx_eikonal_solve(olx_ctx* c, const olx_grid* g, const float* sound_speed, double c_uniform, const double* source_m, double init_radius,
                      int max_sweeps, int* sweeps_out) {
    if (!c) return OLX_EINVAL;
    if (!g || !source_m) return fail(c, OLX_EINVAL, "olx_eikonal_solve: null grid or source");
    for (int a = 0; a < 3; ++a)
        if (g->n[a] < 1 || !(g->spacing[a] > 0) || !std::isfinite(g->spacing[a]) || !std::isfinite(g->origin[a])) return fail(c, OLX_EINVAL, "olx_eikonal_solve: bad grid axis %d", a);
    const long long voxll = (long long)g->n[0] * g->n[1] * g->n[2];
    if (voxll >= (1ll << 31)) return fail(c, OLX_EINVAL, "olx_eikonal_solve: grid of %lld voxels is too large (< 2^31)", voxll);
    if (!(init_radius >= 1) || !std::isfinite(init_radius)) return fail(c, OLX_EINVAL, "olx_eikonal_solve: init_radius must be finite and >= 1");
    if (max_sweeps < 1) return fail(c, OLX_EINVAL, "olx_eikonal_solve: max_sweeps must be >= 1");
    EikonalParams P{};
    P.nx = g->n[0]; P.ny = g->n[1]; P.nz = g->n[2]; P.vox = voxll; P.radius = init_radius;
    for (int a = 0; a < 3; ++a) {
        const double q = (source_m[a] - g->origin[a]) / g->spacing[a];
        if (!(q >= 0 && q <= g->n[a] - 1))
            return fail(c, OLX_EINVAL, "olx_eikonal_solve: the source (%g, %g, %g) m lies outside the grid (axis %d: index %g not in [0, %d])", source_m[0], source_m[1], source_m[2], a, q, g->n[a] - 1);
        P.q[a] = q; P.h[a] = g->spacing[a];
        P.hf[a] = (float)g->spacing[a]; P.wf[a] = (float)(1.0 / (g->spacing[a] * g->spacing[a]));
        P.ilo[a] = (int)std::max(std::ceil(q - init_radius), 0.0);
        P.ihi[a] = (int)std::min(std::floor(q + init_radius), (double)(g->n[a] - 1));
    }
    const size_t vox = (size_t)voxll;
    if (sound_speed) {
        bool bad = false;       // (no early exit: the scan of 16.7 M voxels vectorises, and it is part of every solve with a volume)
        for (size_t o = 0; o < vox; ++o) bad |= !(sound_speed[o] > 0.f && sound_speed[o] <= std::numeric_limits<float>::max());
        if (bad) return fail(c, OLX_EINVAL, "olx_eikonal_solve: sound speed must be finite and > 0");
    } else {
        P.c0 = (float)c_uniform;
        if (!(c_uniform > 0) || !std::isfinite(c_uniform) || !(P.c0 > 0.f) || !std::isfinite(P.c0)) return fail(c, OLX_EINVAL, "olx_eikonal_solve: the uniform sound speed must be finite and > 0");
    }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->ek_solved = false;
    c->ek = P;
    int rc = c->d_ek_T[0].reserve(c, vox);
    if (!rc) rc = c->d_ek_T[1].reserve(c, vox);
    if (!rc) rc = c->d_ek_flag.reserve(c, (size_t)max_sweeps);
    if (!rc && sound_speed) rc = c->d_ek_c.reserve(c, vox);
    if (rc) return rc;
    const float* cs = nullptr;
    if (sound_speed) {
        HIPCHK(c, hipMemcpy(c->d_ek_c, sound_speed, sizeof(float) * vox, hipMemcpyHostToDevice));
        cs = c->d_ek_c;
    }
    HIPCHK(c, hipMemsetAsync(c->d_ek_flag, 0, sizeof(int) * (size_t)max_sweeps, c->stream));
    olx_eikonal_init(c, cs);
    HIPCHK(c, hipGetLastError());
    // no sweep before this one can be the last: until the launch box covers the grid, every sweep reaches new voxels
    int cover = 1;
    for (int a = 0; a < 3; ++a) cover = std::max(cover, std::max(P.ilo[a], g->n[a] - 1 - P.ihi[a]));
    std::vector<int> flags;
    int done = 0, converged = 0;
    while (!converged && done < max_sweeps) {
        const int upto = std::min(max_sweeps, std::max(done + EK_CHECK, cover));
        for (int s = done + 1; s <= upto; ++s) olx_eikonal_sweep(c, cs, s);
        HIPCHK(c, hipGetLastError());
        flags.resize((size_t)(upto - done));
        HIPCHK(c, hipMemcpyAsync(flags.data(), c->d_ek_flag + done, sizeof(int) * flags.size(), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (int s = done + 1; s <= upto && !converged; ++s)
            if (flags[(size_t)(s - done - 1)] == 0) converged = s;
        done = upto;
    }
    if (sweeps_out) *sweeps_out = converged ? converged : done;
    if (!converged) return fail(c, OLX_ENOCONV, "olx_eikonal_solve: no convergence within max_sweeps = %d sweeps", max_sweeps);
    // the sweeps after the first one that changed nothing changed nothing either: both buffers hold the field
    c->ek_cur = done & 1;
    c->ek_solved = true;
    return OLX_OK;
}

int olx_eikonal_sample(olx_ctx* c, int n_points, const int* row, const long long* voxels, const double* weights, double* t_out) {
    if (!c) return OLX_EINVAL;
    if (!c->ek_solved) return fail(c, OLX_ESTATE, "olx_eikonal_sample: no converged olx_eikonal_solve");
    if (n_points < 1 || !row || !t_out) return fail(c, OLX_EINVAL, "olx_eikonal_sample: n_points < 1, or null row table or output");
    if (row[0] != 0) return fail(c, OLX_EINVAL, "olx_eikonal_sample: row[0] must be 0");
    for (int r = 0; r < n_points; ++r)
        if (row[r + 1] < row[r]) return fail(c, OLX_EINVAL, "olx_eikonal_sample: row table not monotone at point %d", r);
    const int n_entries = row[n_points];
    if (n_entries > 0 && (!voxels || !weights)) return fail(c, OLX_EINVAL, "olx_eikonal_sample: null sample table");
    for (int e = 0; e < n_entries; ++e) {
        if (voxels[e] < 0 || voxels[e] >= c->ek.vox) return fail(c, OLX_EINVAL, "olx_eikonal_sample: entry %d: voxel %lld outside the grid of %lld voxels", e, voxels[e], c->ek.vox);
        if (!std::isfinite(weights[e])) return fail(c, OLX_EINVAL, "olx_eikonal_sample: entry %d: weight must be finite", e);
    }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int rc = c->d_ek_row.reserve(c, (size_t)n_points + 1);
    if (!rc) rc = c->d_ek_vox.reserve(c, n_entries);
    if (!rc) rc = c->d_ek_w.reserve(c, n_entries);
    if (!rc) rc = c->d_ek_out.reserve(c, n_points);
    if (rc) return rc;
    HIPCHK(c, hipMemcpy(c->d_ek_row, row, sizeof(int) * ((size_t)n_points + 1), hipMemcpyHostToDevice));
    if (n_entries > 0) {
        HIPCHK(c, hipMemcpy(c->d_ek_vox, voxels, sizeof(long long) * n_entries, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(c->d_ek_w, weights, sizeof(double) * n_entries, hipMemcpyHostToDevice));
    }
    olx_eikonal_sample_launch(c, n_points, n_entries);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
#ifdef OLX_DEBUG_BOUNDS
    { int rc_ = report_bounds(c); if (rc_) return rc_; }
#endif
    return fetch_to_host(c, t_out, c->d_ek_out, sizeof(double) * (size_t)n_points);
}

int olx_eikonal_fetch(olx_ctx* c, float* t_out) {
    if (!c) return OLX_EINVAL;
    if (!c->ek_solved) return fail(c, OLX_ESTATE, "olx_eikonal_fetch: no converged olx_eikonal_solve");
    if (!t_out) return fail(c, OLX_EINVAL, "olx_eikonal_fetch: null output");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
#ifdef OLX_DEBUG_BOUNDS
    { int rc_ = report_bounds(c); if (rc_) return rc_; }
#endif
    return fetch_to_host(c, t_out, c->d_ek_T[c->ek_cur], sizeof(float) * (size_t)c->ek.vox);
}

}  // extern "C"
