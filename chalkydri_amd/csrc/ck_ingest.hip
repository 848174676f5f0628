// ck_ingest.hip — pinned host slots and asynchronous upload in front of the detector.
//
// Mirrors what reaches `AprilTags::process` in the reference: pooled host buffers holding one 8-bit-luma frame each with a
// stride that may exceed the width (crates/chalkydri/src/cameras/gst_to_cu.rs:49-72,131-188; consumed through
// image_from_cuimage, crates/apriltags/src/lib.rs:197-213).  Here a slot is a whole batch: pinned on the host so the copy
// engine reads it directly, laid out exactly like its device twin (16-byte aligned rows) so that ONE asynchronous copy
// moves the batch; the copy runs on its own stream and the compute stream only waits on the slot's event.
#include <string.h>

#include <new>

#include "ck_exposure.h"
#include "ck_internal.h"
#include "ck_jpeg.h"
#include "ck_blobs.h"
#include "ck_preview.h"
#include "ck_raw_planes.h"
#include "ck_rawfmt.h"

struct ck_ingest {
    ck_handle *h;
    int nslots;
    size_t slot_bytes;
    uint8_t *host[8];
    uint8_t *dev[8];
    hipEvent_t ready[8];
    int staged[8];
    hipStream_t copy;
    // a ring of ck_ingest_create_raw: the pinned slots and rawdev[] hold raw frames (rows of geo.stride16, frames of geo.pitch16);
    // submit converts them into dev[], which is luma in the handle's staged layout on either kind of ring
    bool raw;
    ck_raw_format_t fmt;
    ck_raw_geom geo;
    uint8_t *rawdev[8];
    // a ring of ck_ingest_create_jpeg: no pinned luma slots (host[] stays null); the compressed frames, their staging and the decode
    // workspace of every slot live in `jpeg` (ck_jpeg.hip), and submit decodes them into dev[]
    ck_jpeg_slots *jpeg;
    bool pending[8]; // the slot's last submit may still be reading its staging (cleared once ready[slot] has been waited for)
};

static bool slot_ok(const ck_ingest *g, int slot) { return g && slot >= 0 && slot < g->nslots; }
// the slot's luma frames, in the handle's staged layout
static ck_dev_image slot_image(const ck_ingest *g, int slot) { return {g->dev[slot], g->h->frame_stride, g->h->frame_pitch}; }
// the slot's last submit is done: its staging and its workspace are free again
static int wait_slot(ck_ingest *g, int slot) {
    CK_HIP(hipEventSynchronize(g->ready[slot]));
    g->pending[slot] = false;
    return CK_OK;
}
// what the *_ingested calls start with, their arguments checked: the handle's stream waits for the slot's submit
static int await_slot(ck_ingest *g, int slot, ck_dev_image *img) {
    CK_HIP(hipSetDevice(g->h->device));
    if (g->staged[slot] > 0) CK_HIP(hipStreamWaitEvent(g->h->stream, g->ready[slot], 0));
    *img = slot_image(g, slot);
    return CK_OK;
}

// what makes a ring a JPEG ring (nullptr: it is none)
struct jpeg_ring_opts { int32_t orientation; int64_t max_frame_bytes; bool color; };

static int ingest_create(ck_handle_t *h, int32_t n_slots, const ck_raw_format_t *fmt, ck_ingest_t **out, const jpeg_ring_opts *jpeg = nullptr) {
    if (!h || !out || n_slots < 1 || n_slots > 8) return CK_EINVAL;
    *out = nullptr;
    ck_raw_geom geo = {};
    if (fmt) {
        const int rc = ck_raw_geometry(fmt, h->w, h->h, &geo);
        if (rc != CK_OK) return rc;
    }
    CK_HIP(hipSetDevice(h->device));
    ck_ingest *g = new (std::nothrow) ck_ingest();
    if (!g) return CK_ENOMEM;
    memset(g, 0, sizeof *g);
    g->h = h; g->nslots = n_slots;
    const size_t dev_bytes = h->frame_pitch * (size_t)h->cfg.max_batch;
    g->slot_bytes = dev_bytes;
    if (fmt) {
        g->raw = true; g->fmt = *fmt; g->geo = geo;
        g->slot_bytes = geo.pitch16 * (size_t)h->cfg.max_batch;
    }
    hipError_t e = hipStreamCreateWithFlags(&g->copy, hipStreamNonBlocking);
    for (int s = 0; s < n_slots && e == hipSuccess; s++) {
        if (!jpeg) e = hipHostMalloc(reinterpret_cast<void **>(&g->host[s]), g->slot_bytes, hipHostMallocDefault);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&g->dev[s]), dev_bytes);
        if (e == hipSuccess && g->raw) e = hipMalloc(reinterpret_cast<void **>(&g->rawdev[s]), g->slot_bytes);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&g->ready[s], hipEventDisableTiming);
    }
    if (e != hipSuccess) {
        snprintf(ck_err_text, sizeof ck_err_text, "ingest ring allocation failed: %s", hipGetErrorString(e));
        (void)hipGetLastError();
        ck_ingest_destroy(g);
        return CK_ENOMEM;
    }
    if (jpeg) {
        const int rc = ck_jpeg_slots_create(h, n_slots, jpeg->orientation, jpeg->max_frame_bytes, jpeg->color, &g->jpeg);
        if (rc != CK_OK) { ck_ingest_destroy(g); return rc; }
    }
    *out = g;
    return CK_OK;
}

extern "C" int ck_ingest_create_jpeg(ck_handle_t *h, int32_t n_slots, int32_t orientation, int64_t max_frame_bytes, ck_ingest_t **out) {
    if (!ck_orientation_ok(orientation) || max_frame_bytes < 0) return CK_EINVAL;
    const jpeg_ring_opts o = {orientation, max_frame_bytes, false};
    return ingest_create(h, n_slots, nullptr, out, &o);
}

extern "C" int ck_ingest_create_jpeg_color(ck_handle_t *h, int32_t n_slots, int32_t orientation, int64_t max_frame_bytes, ck_ingest_t **out) {
    if (!ck_orientation_ok(orientation) || max_frame_bytes < 0) return CK_EINVAL;
    const jpeg_ring_opts o = {orientation, max_frame_bytes, true};
    return ingest_create(h, n_slots, nullptr, out, &o);
}

extern "C" int ck_ingest_create(ck_handle_t *h, int32_t n_slots, ck_ingest_t **out) { return ingest_create(h, n_slots, nullptr, out); }

extern "C" int ck_ingest_create_raw(ck_handle_t *h, int32_t n_slots, const ck_raw_format_t *fmt, ck_ingest_t **out) {
    if (!fmt) return CK_EINVAL;
    return ingest_create(h, n_slots, fmt, out);
}

extern "C" void ck_ingest_destroy(ck_ingest_t *g) {
    if (!g) return;
    (void)hipSetDevice(g->h->device);
    if (g->copy) (void)hipStreamSynchronize(g->copy);
    for (int s = 0; s < g->nslots; s++) {
        if (g->host[s]) (void)hipHostFree(g->host[s]);
        if (g->dev[s]) (void)hipFree(g->dev[s]);
        if (g->rawdev[s]) (void)hipFree(g->rawdev[s]);
        if (g->ready[s]) (void)hipEventDestroy(g->ready[s]);
    }
    if (g->copy) (void)hipStreamDestroy(g->copy);
    ck_jpeg_slots_free(g->jpeg);
    delete g;
}

extern "C" int32_t ck_ingest_stride(const ck_ingest_t *g) { return !g || g->jpeg ? 0 : g->raw ? g->geo.stride16 : g->h->frame_stride; }

extern "C" uint8_t *ck_ingest_frame(ck_ingest_t *g, int32_t slot, int32_t index) {
    if (!slot_ok(g, slot) || g->jpeg || index < 0 || index >= g->h->cfg.max_batch) return nullptr;
    return g->host[slot] + (size_t)index * (g->raw ? g->geo.pitch16 : g->h->frame_pitch);
}

extern "C" int ck_ingest_write(ck_ingest_t *g, int32_t slot, int32_t index, const ck_image_u8_t *img, uint32_t fourcc) {
    if (g && g->jpeg) return CK_EUNSUPPORTED; // (compressed frames go through ck_ingest_write_jpeg)
    uint8_t *dst = ck_ingest_frame(g, slot, index);
    if (!dst || !img || !img->buf) return CK_EINVAL;
    ck_raw_class cls;
    if (ck_raw_classify(fourcc, &cls) != CK_OK) return CK_EUNSUPPORTED;
    if (g->raw) { // exactly the ring's family, the ring's source geometry, min_stride bytes per row
        const ck_raw_geom &G = g->geo;
        if (!G.planes && cls.bpp == 1) cls.k[0] = 0; // without CK_RAW_PLANES the luma-first fourccs are one family
        if (!ck_raw_same_family(cls, G.cls)) return CK_EUNSUPPORTED;
        if (img->width != G.sw || img->height != G.sh || !ck_raw_stride_ok(G, img->stride)) return CK_EINVAL;
        if (G.planes) { ckp_copy(G.planes, G.sw, G.sh, img->buf, img->stride, dst, G.stride16); return CK_OK; } // all planes
        for (int y = 0; y < G.sh; y++) memcpy(dst + (size_t)y * G.stride16, img->buf + (size_t)y * img->stride, (size_t)G.min_stride);
        return CK_OK;
    }
    if (cls.bpp != 1) return CK_EUNSUPPORTED; // a plain ring takes the formats that start with a luma plane
    const ck_handle *h = g->h;
    if (img->width != h->w || img->height != h->h || img->stride < img->width) return CK_EINVAL;
    for (int y = 0; y < h->h; y++) memcpy(dst + (size_t)y * h->frame_stride, img->buf + (size_t)y * img->stride, (size_t)h->w);
    return CK_OK;
}

extern "C" int ck_ingest_write_jpeg(ck_ingest_t *g, int32_t slot, int32_t index, const uint8_t *data, int64_t size) {
    if (!slot_ok(g, slot) || !g->jpeg || !data || size < 4 || index < 0 || index >= g->h->cfg.max_batch) return CK_EINVAL;
    if (g->pending[slot]) { // (a caller that keeps the header's rule never waits here: the call that processed the slot already has)
        CK_HIP(hipSetDevice(g->h->device));
        const int rc = wait_slot(g, slot);
        if (rc != CK_OK) return rc;
    }
    return ck_jpeg_slots_write(g->jpeg, slot, index, data, size);
}

extern "C" int ck_ingest_jpeg_status(ck_ingest_t *g, int32_t slot, int32_t n, uint32_t *jpeg_status) {
    if (!slot_ok(g, slot) || !g->jpeg || !jpeg_status || n != g->staged[slot]) return CK_EINVAL;
    if (n == 0) return CK_OK;
    CK_HIP(hipSetDevice(g->h->device));
    const int rc = wait_slot(g, slot);
    if (rc != CK_OK) return rc;
    memcpy(jpeg_status, ck_jpeg_slots_status(g->jpeg, slot), sizeof(uint32_t) * (size_t)n);
    return CK_OK;
}

extern "C" int ck_ingest_submit(ck_ingest_t *g, int32_t slot, int32_t n) {
    if (!slot_ok(g, slot) || n < 0 || n > g->h->cfg.max_batch) return CK_EINVAL;
    CK_HIP(hipSetDevice(g->h->device));
    if (g->jpeg) { // head copy, payload copy, decode, oriented IDCT and the status copy, all on the copy stream ahead of the slot's event
        int rc = g->pending[slot] ? wait_slot(g, slot) : CK_OK; // the slot's staging and workspace may still serve its last submit
        if (rc == CK_OK) rc = ck_jpeg_slots_submit(g->jpeg, slot, n, g->copy, slot_image(g, slot));
        if (rc != CK_OK) return rc;
        g->pending[slot] = n > 0;
    } else if (n && g->raw) { // the copy and the conversion both run on the copy stream, ahead of the slot's event
        const ck_raw_geom &G = g->geo;
        CK_HIP(hipMemcpyAsync(g->rawdev[slot], g->host[slot], G.pitch16 * (size_t)n, hipMemcpyHostToDevice, g->copy));
        const int rc = ck_launch_rawfmt(g->h, g->copy, {g->rawdev[slot], G.stride16, G.pitch16, G.sw, G.sh}, G.cls, G.turn, g->dev[slot], n);
        if (rc != CK_OK) return rc;
    } else if (n) CK_HIP(hipMemcpyAsync(g->dev[slot], g->host[slot], g->h->frame_pitch * (size_t)n, hipMemcpyHostToDevice, g->copy));
    CK_HIP(hipEventRecord(g->ready[slot], g->copy));
    g->staged[slot] = n;
    return CK_OK;
}

// `n` is the caller's statement of how many frames its output arrays hold: it must be the count the slot was submitted with
// (the kernels write one entry per staged frame).
extern "C" int ck_detect_ingested(ck_ingest_t *g, int32_t slot, int32_t n, ck_detection_t *dets, int32_t cap, int32_t *counts, uint32_t *status) {
    if (!slot_ok(g, slot) || n != g->staged[slot]) return CK_EINVAL;
    if (n == 0) return CK_OK;
    ck_dev_image img;
    int rc = await_slot(g, slot, &img);
    if (rc == CK_OK) rc = ck_detect_frames(g->h, img, n, dets, cap, counts, status);
    if (rc == CK_OK) g->pending[slot] = false; // (the results are on the host: the stream, and the event it waited for, are done)
    return rc;
}

extern "C" int ck_process_ingested(ck_ingest_t *g, int32_t slot, int32_t n, const ck_process_params_t *pp, const double *gyro,
                                   const uint8_t *has_gyro, ck_vision_measurement_t *out, int32_t *valid) {
    if (!slot_ok(g, slot) || n != g->staged[slot]) return CK_EINVAL;
    if (n == 0) return CK_OK;
    ck_dev_image img;
    int rc = await_slot(g, slot, &img);
    if (rc == CK_OK) rc = ck_process_frames(g->h, img, n, pp, gyro, has_gyro, out, valid);
    if (rc == CK_OK) g->pending[slot] = false;
    return rc;
}

// Exposure metering (ck_exposure.hip) of a submitted slot's frames; the slot stays as it is, so ck_detect_ingested may follow.
extern "C" int ck_exposure_stats_ingested(ck_ingest_t *g, int32_t slot, const int32_t *frames, int32_t n, const ck_exposure_params_t *p,
                                          const ck_rect_t *roi, ck_exposure_stats_t *out) {
    if (!slot_ok(g, slot)) return CK_EINVAL;
    ck_dev_image img;
    const int rc = await_slot(g, slot, &img);
    return rc != CK_OK ? rc : ck_exposure_run(g->h, img, g->staged[slot], frames, n, p, roi, out);
}

// Colour preview (ck_preview.hip) of a submitted slot of a raw ring, from the slot's raw twin: rawdev[slot] keeps the
// frames of the last submit until the slot is submitted again; or (§4i) of a slot of a ring of ck_ingest_create_jpeg_color, whose
// workspace keeps the chroma planes as long.  The slot stays as it is.
static int preview_color_ingested(ck_ingest_t *g, int32_t slot, const ck_preview_params_t *pp, const int32_t *frames, int32_t n,
                                  uint8_t *out, bool files, int64_t cap_per_frame, int64_t *sizes, uint32_t *status) {
    if (!slot_ok(g, slot)) return CK_EINVAL;
    ck_jpeg_color_src js;
    // a plain ring holds luma, a JPEG ring compressed frames: only the ring of ck_ingest_create_jpeg_color keeps their chroma planes
    const bool decoded = g->jpeg && ck_jpeg_slots_color_source(g->jpeg, slot, slot_image(g, slot), g->staged[slot], &js);
    if (!g->raw && !decoded) return CK_EUNSUPPORTED;
    ck_dev_image img;
    const int rc = await_slot(g, slot, &img);
    if (rc != CK_OK) return rc;
    if (decoded) return ck_preview_color_run(g->h, pp, {nullptr, 0, 0, js.n_frames, nullptr, &js}, frames, n, out, files, cap_per_frame, sizes, status);
    return ck_preview_color_run(g->h, pp, {g->rawdev[slot], g->geo.stride16, (int64_t)g->geo.pitch16, g->staged[slot], &g->fmt, nullptr}, frames, n, out,
                                files, cap_per_frame, sizes, status);
}
// Coloured game pieces (ck_blobs.hip) of a submitted slot, from the same sources; the slot stays as it is.
extern "C" int ck_detect_blobs_ingested(ck_ingest_t *g, int32_t slot, const ck_blob_params_t *pp, const int32_t *frames, int32_t n,
                                        ck_blob_t *out, int32_t cap, int32_t *counts, uint32_t *status) {
    if (!slot_ok(g, slot)) return CK_EINVAL;
    ck_jpeg_color_src js;
    const bool decoded = g->jpeg && ck_jpeg_slots_color_source(g->jpeg, slot, slot_image(g, slot), g->staged[slot], &js);
    if (!g->raw && !decoded) return CK_EUNSUPPORTED;
    ck_dev_image img;
    const int rc = await_slot(g, slot, &img);
    if (rc != CK_OK) return rc;
    if (decoded) return ck_blobs_run(g->h, pp, {nullptr, 0, 0, js.n_frames, nullptr, &js}, frames, n, out, cap, counts, status);
    return ck_blobs_run(g->h, pp, {g->rawdev[slot], g->geo.stride16, (int64_t)g->geo.pitch16, g->staged[slot], &g->fmt, nullptr}, frames, n, out,
                        cap, counts, status);
}
extern "C" int ck_preview_jpeg_color_ingested(ck_ingest_t *g, int32_t slot, const ck_preview_params_t *pp, const int32_t *frames, int32_t n,
                                              uint8_t *out, int64_t cap_per_frame, int64_t *sizes, uint32_t *status) {
    return preview_color_ingested(g, slot, pp, frames, n, out, true, cap_per_frame, sizes, status);
}
extern "C" int ck_preview_color_ingested(ck_ingest_t *g, int32_t slot, const ck_preview_params_t *pp, const int32_t *frames, int32_t n,
                                         uint8_t *out) {
    return preview_color_ingested(g, slot, pp, frames, n, out, false, 0, nullptr, nullptr);
}
