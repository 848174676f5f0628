// Coloured game pieces, the host half of the device path: argument checks, the workspace, and the one path of the
// entry points on a colour source (the ring's entry point is in ck_ingest.hip, where the ring is defined).  The kernels are
// k_blobs.hip's, the source is resolved by ck_preview.hip exactly as the colour preview resolves it.
#include "ck_blobs.h"

static_assert(sizeof(ck_blob_class_t) == 56, "ck_blob_class_t layout");
static_assert(sizeof(ck_blob_params_t) == 32 + 4 * 56 + sizeof(ck_camera_t) + sizeof(ck_iso3_t) + 8, "ck_blob_params_t layout");
static_assert(sizeof(ck_blob_t) == 160 && offsetof(ck_blob_t, sx) == 32 && offsetof(ck_blob_t, cx) == 72, "ck_blob_t layout");

namespace {

enum Mode { RGB, MASK, DETECT, TIME };
struct Call {
    Mode mode;
    const ck_blob_params_t *pp;   // null for RGB
    int cls, stage;               // MASK
    void *out;                    // RGB: [n][H][W][3], MASK: [n][H][ww], DETECT: [n][nc][cap]
    int cap; int32_t *counts; uint32_t *status;
    int reps; float *ms;          // TIME
};

// mask + components of one call whose index list is on the device
int enqueue_detect(ck_handle *h, const ck_blob_geom &g, const ck_blob_params_t &pp, const ckb_geo &geo, const ck_pv_src &any, int n) {
    int side;
    const int rc = ck_launch_blob_mask(h, g, pp, any, n, 1, &side);
    return rc != CK_OK ? rc : ck_launch_blob_components(h, g, pp, geo, n, side);
}

int run(ck_handle *h, const ck_pv_color_src &src, const int32_t *frames, int32_t n, const Call &c) {
    if (!h || n < 0 || (c.mode != TIME && !c.out)) return CK_EINVAL;
    if (c.mode != RGB) {
        const int rc = ck_blob_check(c.pp);
        if (rc != CK_OK) return rc;
    }
    if (c.mode == MASK && (c.cls < 0 || c.cls >= c.pp->n_classes || c.stage < 0 || c.stage > 1)) return CK_EINVAL;
    if (c.mode == DETECT && (c.cap < 0 || !c.counts)) return CK_EINVAL;
    if (c.mode == TIME && (c.reps < 1 || !c.ms)) return CK_EINVAL;
    ck_pv_any store;
    ck_pv_src any;
    int n_avail;
    int rc = ck_pv_source(h, src, true, &store, &any, &n_avail);
    if (rc != CK_OK) return rc;
    if (n > h->cfg.max_batch) return CK_ECAPACITY;
    if (!ck_frame_list_ok(frames, n, n_avail)) return CK_EINVAL;
    ck_blob_geom g = {h->w, h->h, (h->w + 31) / 32, c.pp ? c.pp->n_classes : 1, c.pp ? c.pp->max_components : 1, c.mode == DETECT ? c.cap : 0};
    if ((int64_t)g.H * g.ww * 32 >= ((int64_t)1 << 31)) return CK_ECAPACITY; // the run indices are 32-bit
    if ((int64_t)g.maxc > (int64_t)g.W * g.H) g.maxc = g.W * g.H;           // (a plane has no more components than pixels)
    if (n == 0) return CK_OK;
    CK_HIP(hipSetDevice(h->device));
    if (!ck_workspace(h->blobs)) return CK_ENOMEM;
    ck_blob_ws &P = *h->blobs;
    const size_t planes = (size_t)n * g.nc, words = planes * g.H * g.ww;
    rc = P.d_frames.reserve(sizeof(int32_t) * (size_t)n);
    if (rc == CK_OK && c.mode == RGB) rc = P.d_rgb.reserve((size_t)3 * g.W * g.H * n);
    if (rc == CK_OK && c.mode != RGB) rc = P.d_bits.reserve(sizeof(uint32_t) * 2 * words);
    if (rc == CK_OK && c.mode >= DETECT) {
        rc = P.d_parent.reserve(sizeof(uint32_t) * 32 * words);
        if (rc == CK_OK) rc = P.d_area.reserve(sizeof(uint32_t) * 32 * words);
        if (rc == CK_OK) rc = P.d_nslot.reserve(sizeof(uint32_t) * planes);
        if (rc == CK_OK) rc = P.d_comps.reserve(sizeof(ckb_comp) * planes * g.maxc);
        if (rc == CK_OK) rc = P.d_list.reserve(sizeof(uint32_t) * planes * g.maxc);
        if (rc == CK_OK) rc = P.d_out.reserve(sizeof(ck_blob_t) * (planes * g.cap + 1));
        if (rc == CK_OK) rc = P.d_counts.reserve(sizeof(int32_t) * planes);
        if (rc == CK_OK) rc = P.d_status.reserve(sizeof(uint32_t) * (size_t)n);
    }
    if (rc != CK_OK) return rc;
    // the index list: pageable memory, so the copy has read it when the call returns
    {
        int32_t idx_small[64];
        int32_t *idx = n <= 64 ? idx_small : new (std::nothrow) int32_t[n];
        if (!idx) return CK_ENOMEM;
        for (int i = 0; i < n; i++) idx[i] = frames ? frames[i] : i;
        const hipError_t e = hipMemcpyAsync(P.d_frames, idx, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, h->stream);
        const hipError_t e2 = e == hipSuccess ? hipStreamSynchronize(h->stream) : e;
        if (idx != idx_small) delete[] idx;
        CK_HIP(e2);
    }
    if (c.mode == RGB) {
        rc = ck_launch_blob_rgb(h, g, any, n, P.d_rgb);
        if (rc != CK_OK) return rc;
        CK_HIP(hipMemcpyAsync(c.out, P.d_rgb, (size_t)3 * g.W * g.H * n, hipMemcpyDefault, h->stream));
        CK_HIP(hipStreamSynchronize(h->stream));
        return CK_OK;
    }
    if (c.mode == MASK) {
        int side;
        rc = ck_launch_blob_mask(h, g, *c.pp, any, n, c.stage, &side);
        if (rc != CK_OK) return rc;
        // class cls's plane of every frame: n strided pieces of H ww words
        const size_t plane = sizeof(uint32_t) * (size_t)g.H * g.ww;
        const uint8_t *from = reinterpret_cast<const uint8_t *>(P.d_bits.p + (side ? words : 0)) + plane * c.cls;
        CK_HIP(hipMemcpy2DAsync(c.out, plane, from, plane * g.nc, plane, (size_t)n, hipMemcpyDefault, h->stream));
        CK_HIP(hipStreamSynchronize(h->stream));
        return CK_OK;
    }
    ckb_geo geo;
    const ck_camera_t *cam = h->has_camera ? &h->camera : (c.pp->has_camera ? &c.pp->cam : nullptr);
    ckb_geo_make(c.pp, cam, &geo);
    if (c.mode == TIME) {
        for (hipEvent_t &e : P.ev)
            if (!e) CK_HIP(hipEventCreate(&e));
        rc = enqueue_detect(h, g, *c.pp, geo, any, n); // (warm-up: the first launch of a kernel loads its code)
        if (rc != CK_OK) return rc;
        CK_HIP(hipEventRecord(P.ev[0], h->stream));
        for (int r = 0; r < c.reps; r++) {
            rc = enqueue_detect(h, g, *c.pp, geo, any, n);
            if (rc != CK_OK) return rc;
        }
        CK_HIP(hipEventRecord(P.ev[1], h->stream));
        CK_HIP(hipEventSynchronize(P.ev[1]));
        float ms = 0.f;
        CK_HIP(hipEventElapsedTime(&ms, P.ev[0], P.ev[1]));
        *c.ms = ms / (float)c.reps;
        return CK_OK;
    }
    rc = enqueue_detect(h, g, *c.pp, geo, any, n);
    if (rc != CK_OK) return rc;
    if (g.cap) CK_HIP(hipMemcpyAsync(c.out, P.d_out, sizeof(ck_blob_t) * planes * g.cap, hipMemcpyDefault, h->stream));
    CK_HIP(hipMemcpyAsync(c.counts, P.d_counts, sizeof(int32_t) * planes, hipMemcpyDefault, h->stream));
    if (c.status) CK_HIP(hipMemcpyAsync(c.status, P.d_status, sizeof(uint32_t) * (size_t)n, hipMemcpyDefault, h->stream));
    CK_HIP(hipStreamSynchronize(h->stream));
    return CK_OK;
}

int run_staged(ck_handle *h, const int32_t *frames, int32_t n, const Call &c) {
    ck_pv_color_src src;
    ck_jpeg_color_src js;
    const int rc = ck_pv_staged_source(h, &src, &js);
    return rc != CK_OK ? rc : run(h, src, frames, n, c);
}

} // namespace

int ck_blobs_run(ck_handle *h, const ck_blob_params_t *pp, const ck_pv_color_src &src, const int32_t *frames, int32_t n, ck_blob_t *out,
                 int32_t cap, int32_t *counts, uint32_t *status) {
    return run(h, src, frames, n, {DETECT, pp, 0, 0, out, cap, counts, status, 0, nullptr});
}

extern "C" int ck_detect_blobs(ck_handle_t *h, const ck_blob_params_t *pp, const int32_t *frames, int32_t n, ck_blob_t *out, int32_t cap,
                               int32_t *counts, uint32_t *status) {
    return run_staged(h, frames, n, {DETECT, pp, 0, 0, out, cap, counts, status, 0, nullptr});
}
extern "C" int ck_detect_blobs_device(ck_handle_t *h, const ck_blob_params_t *pp, const uint8_t *d_raw, int32_t stride, int64_t frame_pitch,
                                      const ck_raw_format_t *fmt, const int32_t *frames, int32_t n_frames, int32_t n, ck_blob_t *out,
                                      int32_t cap, int32_t *counts, uint32_t *status) {
    return ck_blobs_run(h, pp, {d_raw, stride, frame_pitch, n_frames, fmt, nullptr}, frames, n, out, cap, counts, status);
}
extern "C" int ck_blob_rgb(ck_handle_t *h, const int32_t *frames, int32_t n, uint8_t *rgb_out) {
    return run_staged(h, frames, n, {RGB, nullptr, 0, 0, rgb_out, 0, nullptr, nullptr, 0, nullptr});
}
extern "C" int ck_blob_rgb_device(ck_handle_t *h, const uint8_t *d_raw, int32_t stride, int64_t frame_pitch, const ck_raw_format_t *fmt,
                                  const int32_t *frames, int32_t n_frames, int32_t n, uint8_t *rgb_out) {
    return run(h, {d_raw, stride, frame_pitch, n_frames, fmt, nullptr}, frames, n, {RGB, nullptr, 0, 0, rgb_out, 0, nullptr, nullptr, 0, nullptr});
}
extern "C" int ck_blob_mask(ck_handle_t *h, const ck_blob_params_t *pp, const int32_t *frames, int32_t n, int32_t cls, int32_t stage,
                            uint32_t *bits_out) {
    return run_staged(h, frames, n, {MASK, pp, cls, stage, bits_out, 0, nullptr, nullptr, 0, nullptr});
}
extern "C" int ck_blob_mask_device(ck_handle_t *h, const ck_blob_params_t *pp, const uint8_t *d_raw, int32_t stride, int64_t frame_pitch,
                                   const ck_raw_format_t *fmt, const int32_t *frames, int32_t n_frames, int32_t n, int32_t cls,
                                   int32_t stage, uint32_t *bits_out) {
    return run(h, {d_raw, stride, frame_pitch, n_frames, fmt, nullptr}, frames, n, {MASK, pp, cls, stage, bits_out, 0, nullptr, nullptr, 0, nullptr});
}
extern "C" int ck_blob_time(ck_handle_t *h, const ck_blob_params_t *pp, const uint8_t *d_raw, int32_t stride, int64_t frame_pitch,
                            const ck_raw_format_t *fmt, int32_t n_frames, int32_t n, int32_t reps, float *ms_out) {
    return run(h, {d_raw, stride, frame_pitch, n_frames, fmt, nullptr}, nullptr, n, {TIME, pp, 0, 0, nullptr, 0, nullptr, nullptr, reps, ms_out});
}
