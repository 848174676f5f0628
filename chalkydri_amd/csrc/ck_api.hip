// ck_api.hip — C ABI entry points: handle lifecycle, frame staging, stage orchestration.
// See include/chalkydri_hip.h for the contract and the reference interfaces each entry replaces.
#include <string.h>

#include <new>
#include <vector>

#include "ck_exposure.h"
#include "ck_internal.h"
#include "ck_jpeg.h"
#include "ck_preview.h"
#include "ck_rawfmt.h"
#include "ck_tri_otsu.h"
#include "ck_calib.h"
#include "ck_rig.h"
#include "ck_rigcal.h"
#include "ck_fieldcal.h"
#include "ck_rig_refine.h"
#include "ck_blobs.h"
#include "ck_subpix.h"

thread_local char ck_err_text[512] = "";

// ---- CK_POISON=3: guard-page allocations (ck_internal.h) --------------------------------------------------------------------------
#include <map>
#include <mutex>
namespace {
std::mutex g_guard_mu;
std::map<void *, ck_guarded_alloc> g_guarded;
}
hipError_t ck_guarded_malloc(void **p, size_t bytes) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    hipMemAllocationProp prop = {};
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = dev;
    size_t gran = 0;
    e = hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityMinimum);
    if (e != hipSuccess || gran == 0) return e != hipSuccess ? e : hipErrorUnknown;
    ck_guarded_alloc g = {};
    const size_t used = (bytes + 15) / 16 * 16;                    // the buffer keeps 16-byte alignment (its widest accesses); at most 15 bytes of slack
    g.map_bytes = (used + gran - 1) / gran * gran;
    g.va_bytes = g.map_bytes + gran;                               // ... and one granule that stays unmapped
    e = hipMemAddressReserve(&g.va, g.va_bytes, gran, nullptr, 0);
    if (e != hipSuccess) return e;
    e = hipMemCreate(&g.mem, g.map_bytes, &prop, 0);
    if (e != hipSuccess) { (void)hipMemAddressFree(g.va, g.va_bytes); return e; }
    e = hipMemMap(g.va, g.map_bytes, 0, g.mem, 0);
    hipMemAccessDesc acc = {};
    acc.location = prop.location;
    acc.flags = hipMemAccessFlagsProtReadWrite;
    if (e == hipSuccess) e = hipMemSetAccess(g.va, g.map_bytes, &acc, 1);
    if (e != hipSuccess) { (void)hipMemRelease(g.mem); (void)hipMemAddressFree(g.va, g.va_bytes); return e; }
    *p = static_cast<char *>(g.va) + (g.map_bytes - used);
    std::lock_guard<std::mutex> lk(g_guard_mu);
    g_guarded[*p] = g;
    return hipSuccess;
}
bool ck_guarded_free(void *p) {
    ck_guarded_alloc g;
    {
        std::lock_guard<std::mutex> lk(g_guard_mu);
        auto it = g_guarded.find(p);
        if (it == g_guarded.end()) return false;
        g = it->second;
        g_guarded.erase(it);
    }
    (void)hipDeviceSynchronize();
    (void)hipMemUnmap(g.va, g.map_bytes);
    (void)hipMemRelease(g.mem);
    // The address range stays reserved for the life of the process.  Freed, the runtime hands the same range to the next
    // reservation, and kernels then still reach the OLD, released pages through it while the copy engine sees the new ones
    // (tools/probes/vmm_reuse_probe.hip shows it with runtime calls alone: every reuse reads back zeros / the fill pattern):
    // that was the fp64 probe's "zeros" under CK_POISON=3.  A test process reserves a few thousand ranges of 47-bit address
    // space at most; and an access after free faults now, too.
    return true;
}

extern "C" const char *ck_last_error(void) { return ck_err_text; }

int ck_hip_failed(hipError_t e, const char *call, const char *file, int line, bool alloc) {
    snprintf(ck_err_text, sizeof ck_err_text, "%s failed: %s (%s:%d)", call, hipGetErrorString(e), file, line);
    (void)hipGetLastError();
    return alloc && e == hipErrorOutOfMemory ? CK_ENOMEM : CK_EDEVICE;
}

extern "C" int ck_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

static int round_up(int v, int m) { return (v + m - 1) / m * m; }

// The rules beside ck_family_t in chalkydri_hip.h.  k_decode relies on them: 8 * width_at_border border samples and the
// total_width^2 grid live in fixed LDS arrays, every bit cell is written into that grid, a code word is one lane's register
// of at most 64 bits, and the codebook search packs the id into 20 bits of its key.
static bool family_ok(const ck_family_t *f) {
    if (!f) return false;
    if (!f->codes || !f->bit_x || !f->bit_y) return false;
    if (f->nbits < 1) return false;
    if (f->nbits > 64) return false;
    if (f->ncodes < 1) return false;
    if (f->ncodes >= (1u << 20)) return false;
    if (f->n_upstream > f->ncodes) return false;
    if (f->width_at_border < 1) return false;
    if (f->total_width > 16) return false;
    if (f->width_at_border > f->total_width) return false;
    const int min_coord = (f->width_at_border - f->total_width) / 2; // (k_decode's and AprilTag-3's)
    for (uint32_t i = 0; i < f->nbits; i++) {
        const int x = (int)f->bit_x[i], y = (int)f->bit_y[i];
        if (x < min_coord || x >= min_coord + f->total_width || y < min_coord || y >= min_coord + f->total_width) return false;
    }
    if (f->nbits < 64)
        for (uint32_t k = 0; k < f->ncodes; k++)
            if (f->codes[k] >> f->nbits) return false;
    return true;
}

// streams, events and buffers of a new handle; what fails here for lack of memory is CK_ENOMEM, whichever call it is
static int create_device_side(ck_handle *h) {
    CK_HIP_ALLOC(hipSetDevice(h->device));
    CK_HIP_ALLOC(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    for (auto &e : h->ev) CK_HIP_ALLOC(hipEventCreate(&e));
    CK_HIP_ALLOC(hipEventCreateWithFlags(&h->ev_fit_fork, hipEventDisableTiming));
    for (auto &st : h->fit_stream) CK_HIP_ALLOC(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    for (auto &e : h->ev_fit_join) CK_HIP_ALLOC(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return ck_bufs_create(h);
}

extern "C" int ck_create(const ck_config_t *cfg, ck_handle_t **out) {
    if (!cfg || !out) return CK_EINVAL;
    *out = nullptr;
    if (cfg->width < 16 || cfg->height < 16 || cfg->width > 4095 || cfg->height > 4095) return CK_EINVAL;
    if (cfg->max_batch < 1 || cfg->n_families < 1 || cfg->n_families > CK_MAX_FAMILIES) return CK_EINVAL;
    if (cfg->quad_decimate != 1 && cfg->quad_decimate != 2) return CK_EUNSUPPORTED;
    for (int i = 0; i < cfg->n_families; i++)
        if (!family_ok(cfg->families[i])) return CK_EINVAL;
    int qw = cfg->width / cfg->quad_decimate, qh = cfg->height / cfg->quad_decimate;
    if (qw < 8 || qh < 8) return CK_EINVAL;
    if (cfg->min_component_px < 1 || cfg->min_component_px > 0x3FFFFFFF) return CK_EINVAL;
    // k_finalize ranks a frame's decode candidates (one per quad and family) in dynamic LDS, 4 bytes each, and raises no limit for
    // it: 64 KiB is what a launch is given without hipFuncSetAttribute (CK_MAX_FRAME_CANDIDATES; stage_caps holds the same bound)
    if ((long long)(cfg->max_quads_per_frame > 0 ? cfg->max_quads_per_frame : 1024) * cfg->n_families > CK_MAX_FRAME_CANDIDATES) return CK_EINVAL;
    if (ck_device_count() <= 0) return CK_ENODEVICE;
    ck_handle *h = new (std::nothrow) ck_handle();
    if (!h) return CK_ENOMEM;
    memset(h, 0, sizeof *h);
    h->cfg = *cfg;
    h->device = cfg->device;
    h->n_last_pose = -1;
    h->n_raw_staged = -1;
    h->n_jpeg_color = -1;
    h->n_last_dets = -1;
    h->n_pose_inputs = -1;
    h->w = cfg->width; h->h = cfg->height; h->qw = qw; h->qh = qh;
    h->npix = (size_t)qw * qh;
    h->tiles_x = (qw + CK_TW - 1) / CK_TW; h->tiles_y = (qh + CK_TH - 1) / CK_TH;
    h->broot_cap = h->tiles_x * h->tiles_y * CK_RING_CAP;
    h->ring_len = (2 * ((size_t)h->tiles_y * qw + (size_t)h->tiles_x * qh) + 3) & ~(size_t)3; // frames stay 8-byte aligned
    h->frame_stride = round_up(cfg->width, 16);
    h->frame_pitch = (size_t)h->frame_stride * cfg->height;
    const int rc = create_device_side(h);
    if (rc != CK_OK) { ck_destroy(h); return rc; }
    *out = h;
    return CK_OK;
}

extern "C" void ck_destroy(ck_handle_t *h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (auto &st : h->fit_stream) if (st) (void)hipStreamSynchronize(st);
    ck_bufs_free(h);
    delete h->jpeg; // the on-demand workspaces own their buffers (ck_grow.h)
    delete h->raw;
    delete h->preview;
    delete h->exposure;
    delete h->tri_otsu;
    delete h->calib;
    delete h->rig;
    delete h->rigcal;
    delete h->fieldcal;
    delete h->rig_refine;
    delete h->blobs;
    delete h->subpix_ws;
    for (auto &e : h->ev) if (e) (void)hipEventDestroy(e);
    if (h->ev_fit_fork) (void)hipEventDestroy(h->ev_fit_fork);
    for (auto &e : h->ev_fit_join) if (e) (void)hipEventDestroy(e);
    for (auto &st : h->fit_stream) if (st) (void)hipStreamDestroy(st);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    (void)hipGetLastError(); // (what the clean-up calls above may have left behind — a handle that never got its device, say — is not the next call's error)
}

int ck_read_staged_luma(ck_handle *h, int n, uint8_t *luma_out) {
    if (n) CK_HIP(hipMemcpy2DAsync(luma_out, (size_t)h->w, h->d_frames, (size_t)h->frame_stride, (size_t)h->w, (size_t)h->h * n,
                                   hipMemcpyDeviceToHost, h->stream));
    return CK_OK;
}

static int check_imgs(const ck_handle *h, const ck_image_u8_t *imgs, int n) {
    if (n < 0 || (n > 0 && !imgs)) return CK_EINVAL;
    if (n > h->cfg.max_batch) return CK_ECAPACITY;
    for (int i = 0; i < n; i++)
        if (!imgs[i].buf || imgs[i].width != h->w || imgs[i].height != h->h || imgs[i].stride < imgs[i].width) return CK_EINVAL;
    return CK_OK;
}

extern "C" int ck_upload_frames(ck_handle_t *h, const ck_image_u8_t *imgs, int32_t n) {
    if (!h) return CK_EINVAL;
    int rc = check_imgs(h, imgs, n);
    if (rc != CK_OK) return rc;
    CK_HIP(hipSetDevice(h->device));
    for (int i = 0; i < n; i++)
        CK_HIP(hipMemcpy2DAsync(h->d_frames + (size_t)i * h->frame_pitch, (size_t)h->frame_stride, imgs[i].buf, (size_t)imgs[i].stride,
                                (size_t)h->w, (size_t)h->h, hipMemcpyHostToDevice, h->stream));
    CK_HIP(hipStreamSynchronize(h->stream));
    ck_set_staged(h, n);
    return CK_OK;
}

// Makes d_frames hold a 16-byte aligned copy of caller-resident device frames when their layout is not directly usable.
int ck_stage_device_frames(ck_handle *h, const uint8_t *d_frames, int n, int stride, int64_t frame_pitch, ck_dev_image *use) {
    if (!d_frames || n < 0 || stride < h->w || frame_pitch < (int64_t)stride * h->h) return CK_EINVAL;
    if (n > h->cfg.max_batch) return CK_ECAPACITY;
    bool aligned = ((uintptr_t)d_frames % 16 == 0) && (stride % 16 == 0) && (frame_pitch % 16 == 0);
    if (aligned) { *use = {d_frames, stride, (size_t)frame_pitch}; return CK_OK; }
    for (int i = 0; i < n; i++)
        CK_HIP(hipMemcpy2DAsync(h->d_frames + (size_t)i * h->frame_pitch, (size_t)h->frame_stride, d_frames + (size_t)i * frame_pitch,
                                (size_t)stride, (size_t)h->w, (size_t)h->h, hipMemcpyDeviceToDevice, h->stream));
    ck_set_staged(h, n);
    *use = ck_staged_image(h);
    return CK_OK;
}

// Q of n frames into d_qframes when the quad image is a buffer of its own: decimation and / or the quad_sigma filter
int ck_make_quad_image(ck_handle *h, const ck_dev_image &img, int n) {
    if (!ck_quad_separate(h)) return CK_OK;
    return h->qf_ksz > 1 ? ck_launch_prefilter(h, img, n) : ck_launch_decimate(h, img, n);
}

// Runs that (if configured) + threshold + segment on n staged frames.
int ck_run_threshold_segment(ck_handle *h, const ck_dev_image &img, int n) {
    int rc = ck_make_quad_image(h, img, n);
    if (rc != CK_OK) return rc;
    return ck_launch_threshold_segment(h, ck_quad_image(h, img), n);
}

static int stage_input(ck_handle *h, const ck_image_u8_t *imgs, int n) {
    if (imgs) return ck_upload_frames(h, imgs, n);
    if (n < 0 || n > h->n_staged) return CK_EINVAL;
    return CK_OK;
}

extern "C" int ck_threshold_batch(ck_handle_t *h, const ck_image_u8_t *imgs, int32_t n, uint8_t *thresh_out) {
    if (!h || !thresh_out) return CK_EINVAL;
    int rc = stage_input(h, imgs, n);
    if (rc != CK_OK) return rc;
    CK_HIP(hipSetDevice(h->device));
    rc = ck_run_threshold_segment(h, ck_staged_image(h), n);
    if (rc != CK_OK) return rc;
    CK_HIP(hipMemcpyAsync(thresh_out, h->d_thresh, h->npix * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    CK_HIP(hipStreamSynchronize(h->stream));
    return CK_OK;
}

extern "C" int ck_segment_batch(ck_handle_t *h, const ck_image_u8_t *imgs, int32_t n, uint32_t *labels_out, uint32_t *sizes_out) {
    if (!h || !labels_out) return CK_EINVAL;
    int rc = stage_input(h, imgs, n);
    if (rc != CK_OK) return rc;
    CK_HIP(hipSetDevice(h->device));
    rc = ck_run_threshold_segment(h, ck_staged_image(h), n);
    if (rc != CK_OK) return rc;
    size_t total = h->npix * (size_t)n;
    uint32_t *d_canon = nullptr, *d_sizes = nullptr;
    auto fetch = [&]() -> int {
        int r = ck_launch_canonical_labels(h, n, d_canon, d_sizes);
        if (r != CK_OK) return r;
        CK_HIP(hipMemcpyAsync(labels_out, d_canon, total * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        if (sizes_out) CK_HIP(hipMemcpyAsync(sizes_out, d_sizes, total * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        CK_HIP(hipStreamSynchronize(h->stream));
        return CK_OK;
    };
    hipError_t e = ck_malloc_dev(&d_canon, total * sizeof(uint32_t));
    if (e == hipSuccess && sizes_out) e = ck_malloc_dev(&d_sizes, total * sizeof(uint32_t));
    if (e == hipSuccess) rc = fetch();
    else { (void)ck_hip_failed(e, "ck_malloc_dev(label arrays)", __FILE__, __LINE__, true); rc = CK_ENOMEM; } // (here any failed allocation is CK_ENOMEM)
    (void)ck_free_dev(d_canon); (void)ck_free_dev(d_sizes); // one exit: nothing leaks on an error path
    return rc;
}

extern "C" int ck_set_quad_sigma(ck_handle_t *h, float sigma) {
    if (!h) return CK_EINVAL;
    uint8_t k[33];
    int32_t ksz = 1;
    int rc = ck_quad_sigma_kernel(sigma, k, 33, &ksz);
    if (rc != CK_OK) return rc;
    if (ksz > 1 && !h->d_qframes) { // quad_decimate 1: the quad image becomes a buffer of its own the first time the filter is on
        CK_HIP(hipSetDevice(h->device));
        rc = ck_buf_alloc(h, &h->d_qframes);
        if (rc != CK_OK) return rc;
    }
    h->quad_sigma = sigma;
    h->qf_ksz = ksz;
    memcpy(h->qf_k, k, sizeof h->qf_k);
    return CK_OK;
}

extern "C" int ck_quad_image_batch(ck_handle_t *h, const ck_image_u8_t *imgs, int32_t n, uint8_t *out) {
    if (!h || !out) return CK_EINVAL;
    int rc = stage_input(h, imgs, n);
    if (rc != CK_OK) return rc;
    if (n == 0) return CK_OK;
    CK_HIP(hipSetDevice(h->device));
    rc = ck_make_quad_image(h, ck_staged_image(h), n);
    if (rc != CK_OK) return rc;
    const ck_dev_image q = ck_quad_image(h, ck_staged_image(h));
    for (int i = 0; i < n; i++)
        CK_HIP(hipMemcpy2DAsync(out + (size_t)i * h->npix, (size_t)h->qw, q.p + (size_t)i * q.pitch, (size_t)q.stride, (size_t)h->qw, (size_t)h->qh,
                                hipMemcpyDeviceToHost, h->stream));
    CK_HIP(hipStreamSynchronize(h->stream));
    return CK_OK;
}

extern "C" int ck_time_threshold_segment(ck_handle_t *h, int32_t n, int32_t iters, float *ms_out) {
    if (!h || !ms_out || iters < 1 || n < 1 || n > h->n_staged) return CK_EINVAL;
    CK_HIP(hipSetDevice(h->device));
    int rc = ck_run_threshold_segment(h, ck_staged_image(h), n); // warm-up
    if (rc != CK_OK) return rc;
    CK_HIP(hipEventRecord(h->ev[0], h->stream));
    for (int i = 0; i < iters; i++) {
        rc = ck_run_threshold_segment(h, ck_staged_image(h), n);
        if (rc != CK_OK) return rc;
    }
    CK_HIP(hipEventRecord(h->ev[1], h->stream));
    CK_HIP(hipEventSynchronize(h->ev[1]));
    float ms = 0;
    CK_HIP(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
    *ms_out = ms / (float)iters;
    return CK_OK;
}

extern "C" int ck_last_stage_ms(ck_handle_t *h, ck_stage_ms_t *out) {
    if (!h || !out) return CK_EINVAL;
    *out = h->last_ms;
    return CK_OK;
}

// fp64 conformance probe ------------------------------------------------------------------------------------------
__global__ void k_fp64_probe(int op, const double *a, const double *b, int n, double *out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double x = a[i], y = b ? b[i] : 0.0, r;
    switch (op) {
    case 0: r = x + y; break;
    case 1: r = x * y; break;
    case 2: r = x / y; break;
    case 3: r = sqrt(x); break;
    default: { double t = x * y; r = t + x; } break;
    }
    out[i] = r;
}
extern "C" int ck_selftest_fp64(ck_handle_t *h, int32_t op, const double *a, const double *b, int32_t n, double *out) {
    if (!h || !a || !out || n < 0) return CK_EINVAL;
    CK_HIP(hipSetDevice(h->device));
    if (n == 0) return CK_OK;
    double *da = nullptr, *db = nullptr, *dout = nullptr;
    const size_t bytes = sizeof(double) * (size_t)n;
    auto run = [&]() -> int { // (every failure of the probe, its allocations included, is CK_EDEVICE)
        CK_HIP(ck_malloc_dev(&da, bytes));
        CK_HIP(ck_malloc_dev(&dout, bytes));
        if (b) CK_HIP(ck_malloc_dev(&db, bytes));
        CK_HIP(hipMemcpy(da, a, bytes, hipMemcpyHostToDevice));
        if (b) CK_HIP(hipMemcpy(db, b, bytes, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_fp64_probe, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, op, da, db, n, dout);
        CK_HIP(hipStreamSynchronize(h->stream));
        CK_HIP(hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost));
        return CK_OK;
    };
    const int rc = run();
    (void)ck_free_dev(da); (void)ck_free_dev(db); (void)ck_free_dev(dout); // one exit: nothing leaks on an error path
    return rc;
}
