// ck_stages.hip — the handle's device buffers (one table: allocation, release, the names CK_POISON=2 prints) and the
// detect / clusters / quads / process entry points.
#include <string.h>

#include <vector>

#include "ck_internal.h"
#include "ck_subpix.h"

static int next_pow2(int v) { int p = 1; while (p < v) p <<= 1; return p; }

// ---- the handle's device buffers ---------------------------------------------------------------------------------------------
// Every device buffer of ck_handle / ck_stage_ws is one row of ck_bufs[]: allocation (ck_bufs_create in this order; ck_buf_alloc
// for the ones allocated on first use), release (ck_bufs_free) and the name CK_POISON=2 prints all walk this table.  A new buffer
// is a member + a row; ck_jpeg_ws and ck_raw_ws (grown per call) keep their own.
enum : unsigned {
    CK_BUF_FRAME = 1, // [max_batch][bytes]
    CK_BUF_LAZY = 4,  // not allocated by ck_create (d_qframes: at quad_decimate 2 it is)
    CK_BUF_ALIAS = 8, // the row before it seen as another type: same storage, same pitch in bytes; not allocated, not freed
};
struct ck_buf_desc {
    const char *name;
    size_t member;                     // offsetof(ck_handle, the pointer)
    unsigned flags;                    // (none: one array of `bytes` per handle)
    size_t (*bytes)(const ck_handle *); // per frame / in all; 0: this handle has no such buffer
};
#define CK_BUF(member, flags, expr) \
    {#member, offsetof(ck_handle, member), flags, [](const ck_handle *h) -> size_t { const ck_stage_ws &w = h->ws; (void)w; return (size_t)(expr); }}
static size_t fam_codes_bytes(const ck_handle *h) {
    size_t n = 0;
    for (int f = 0; f < h->cfg.n_families; f++) n += h->cfg.families[f]->ncodes;
    return n * sizeof(uint64_t);
}
static constexpr ck_buf_desc ck_bufs[] = {
    CK_BUF(d_frames, CK_BUF_FRAME, h->frame_pitch),
    CK_BUF(d_qframes, CK_BUF_FRAME | CK_BUF_LAZY, ck_qframes_image(h).pitch),
    CK_BUF(d_thresh, CK_BUF_FRAME, h->npix),
    CK_BUF(d_labels, CK_BUF_FRAME, h->npix * sizeof(ck_label_t)),
    CK_BUF(d_groot, CK_BUF_FRAME, h->broot_cap * sizeof(uint32_t)),
    CK_BUF(d_gsize, CK_BUF_FRAME, h->broot_cap * sizeof(uint32_t)),
    CK_BUF(d_gscratch, CK_BUF_FRAME, 2 * h->broot_cap * sizeof(uint32_t)),
    CK_BUF(d_xband, CK_BUF_FRAME, 2 * h->broot_cap * sizeof(uint32_t)),
    CK_BUF(d_broots, CK_BUF_FRAME, 2 * h->broot_cap * sizeof(ck_border_root)),
    CK_BUF(d_tile_count, CK_BUF_FRAME, (size_t)h->tiles_x * h->tiles_y * sizeof(uint32_t)),
    CK_BUF(d_ring, CK_BUF_FRAME, h->ring_len * sizeof(uint16_t)),
    CK_BUF(ws.d_ht_keys, CK_BUF_FRAME, w.ht_size * sizeof(unsigned long long)),
    CK_BUF(ws.d_ht_count, CK_BUF_FRAME, w.ht_size * sizeof(unsigned long long)),
    CK_BUF(ws.d_ht_off, CK_BUF_FRAME, w.ht_size * sizeof(uint32_t)),
    CK_BUF(ws.d_tmp, CK_BUF_FRAME, w.ext_cap * sizeof(ck_packed_point)),
    CK_BUF(ws.d_ext_xy, CK_BUF_FRAME | CK_BUF_ALIAS, w.ext_cap * sizeof(uint32_t)),
    CK_BUF(ws.d_points, CK_BUF_FRAME, w.ext_cap * sizeof(ck_packed_point)),
    CK_BUF(ws.d_maxval, CK_BUF_FRAME | CK_BUF_ALIAS, (w.ext_cap / 2) * sizeof(double)),
    CK_BUF(ws.d_ext_w, CK_BUF_FRAME, w.ext_cap * sizeof(uint16_t)),
    CK_BUF(ws.d_maxpos, CK_BUF_FRAME, (w.ext_cap / 2) * sizeof(uint16_t)),
    CK_BUF(ws.d_maxmask, CK_BUF_FRAME, (w.ext_cap / 64) * sizeof(unsigned long long)),
    CK_BUF(ws.d_maxpre, CK_BUF_FRAME, (w.ext_cap / 64) * sizeof(uint16_t)),
    CK_BUF(ws.d_blk, CK_BUF_FRAME, 6 * (size_t)(w.ext_cap / 32) * sizeof(long long)),
    CK_BUF(ws.d_cstate, CK_BUF_FRAME, 2 * w.cluster_cap * sizeof(uint32_t)),
    CK_BUF(ws.d_runs, CK_BUF_FRAME, w.run_cap * sizeof(ck_run)),
    CK_BUF(ws.d_lscratch, 0, sizeof(unsigned long long) * CK_LSCRATCH_PER_WG * CK_LSCRATCH_WGS),
    // (1920 x 1080: 18 432 points, 144 MiB instead of the 512 MiB of the class's template capacity)
    CK_BUF(ws.d_hscratch, 0, w.max_cluster_points > 16384 ? sizeof(unsigned long long) * 2 * w.hcap * CK_HUGE_WGS : 0),
    CK_BUF(ws.d_clusters, CK_BUF_FRAME, w.cluster_cap * sizeof(ck_cluster_t)),
    CK_BUF(ws.d_counters, CK_BUF_FRAME, CK_CNT_STRIDE * sizeof(uint32_t)),
    CK_BUF(ws.d_quads, CK_BUF_FRAME, w.quad_cap * sizeof(ck_quad_t)),
    CK_BUF(ws.d_dets, CK_BUF_FRAME, w.det_cap * sizeof(ck_detection_t)),
    CK_BUF(ws.d_fit_scratch, 0, w.fit_scratch_bytes),
    CK_BUF(ws.d_wimg, CK_BUF_FRAME, h->npix * sizeof(uint16_t)),
    CK_BUF(ws.d_field, 0, w.field_cap * sizeof(ck_field_tag_t)),
    CK_BUF(ws.d_gyro, CK_BUF_FRAME, sizeof(double)),
    CK_BUF(ws.d_has_gyro, CK_BUF_FRAME, 1),
    CK_BUF(ws.d_problems, CK_BUF_FRAME, sizeof(ck_sqpnp_problem_t)),
    CK_BUF(ws.d_pose_tags, CK_BUF_FRAME, w.det_cap * sizeof(ck_iso3_t)),
    CK_BUF(ws.d_bearings, CK_BUF_FRAME, w.det_cap * 12 * sizeof(double)),
    CK_BUF(ws.d_world, CK_BUF_FRAME, w.det_cap * 12 * sizeof(double)),
    CK_BUF(ws.d_results, CK_BUF_FRAME, sizeof(ck_sqpnp_result_t)),
    CK_BUF(ws.d_meas, CK_BUF_FRAME, sizeof(ck_vision_measurement_t)),
    CK_BUF(ws.d_valid, CK_BUF_FRAME, sizeof(int32_t)),
    CK_BUF(d_fam_codes, 0, fam_codes_bytes(h)),
    CK_BUF(d_fams, 0, h->cfg.n_families * sizeof(ck_dev_family)),
    // per-tag pose (k_tagpose.hip), by the first call that needs them; one call's records, max_batch * det_cap of them
    CK_BUF(d_tp_dets, CK_BUF_LAZY, (size_t)h->cfg.max_batch * w.det_cap * sizeof(ck_detection_t)),
    CK_BUF(d_tp_counts, CK_BUF_LAZY, h->cfg.max_batch * sizeof(int32_t)),
    CK_BUF(d_tp_out, CK_BUF_LAZY, (size_t)h->cfg.max_batch * w.det_cap * sizeof(ck_tag_pose_t)),
};
#undef CK_BUF
// A pointer added to ck_stage_ws without a row above stops the build here (so does any other member: then correct the 64 bytes
// that its capacities and their padding take)
constexpr int ws_rows() {
    int n = 0;
    for (const ck_buf_desc &d : ck_bufs) n += d.member >= offsetof(ck_handle, ws) && d.member < offsetof(ck_handle, ws) + sizeof(ck_stage_ws);
    return n;
}
static_assert(sizeof(ck_stage_ws) == ws_rows() * sizeof(void *) + 64, "every pointer of ck_stage_ws has one row in ck_bufs[]");

static char *&buf_ptr(ck_handle *h, const ck_buf_desc &d) { return *reinterpret_cast<char **>(reinterpret_cast<char *>(h) + d.member); }

static int alloc_one(ck_handle *h, const ck_buf_desc &d) {
    if (d.flags & CK_BUF_ALIAS) { buf_ptr(h, d) = buf_ptr(h, (&d)[-1]); return CK_OK; }
    const size_t bytes = d.bytes(h) * (d.flags & CK_BUF_FRAME ? (size_t)h->cfg.max_batch : 1);
    if (!bytes || buf_ptr(h, d)) return CK_OK;
    CK_HIP_ALLOC(ck_malloc_dev_at(&buf_ptr(h, d), bytes, d.name, __LINE__)); // (a buffer whose fill failed is still the handle's: ck_bufs_free)
    return CK_OK;
}

int ck_buf_alloc(ck_handle *h, const void *member) {
    for (const ck_buf_desc &d : ck_bufs)
        if (reinterpret_cast<const char *>(h) + d.member == member) return alloc_one(h, d);
    return CK_EINVAL;
}

void ck_bufs_free(ck_handle *h) {
    for (const ck_buf_desc &d : ck_bufs)
        if (!(d.flags & CK_BUF_ALIAS)) (void)ck_free_dev(buf_ptr(h, d));
}

// capacities of the workspace of the irregular stages, from the configuration
static int stage_caps(ck_handle *h) {
    ck_stage_ws &ws = h->ws;
    const ck_config_t &cfg = h->cfg;
    const size_t nb = (size_t)cfg.max_batch;
    const int npix = (int)h->npix;
    ws.point_cap = cfg.max_points_per_frame > 0 ? cfg.max_points_per_frame : 4 * npix; // a pixel has four forward neighbours: no frame has more
    ws.cluster_cap = cfg.max_clusters_per_frame > 0 ? cfg.max_clusters_per_frame : npix / 32;
    if (ws.cluster_cap < 1024) ws.cluster_cap = 1024;
    if (ws.cluster_cap > (1 << 19)) ws.cluster_cap = 1 << 19; // keeps the hash table (2x) at most 2^20 slots per frame
    ws.quad_cap = cfg.max_quads_per_frame > 0 ? cfg.max_quads_per_frame : 1024;
    // k_finalize ranks a frame's decode candidates (quad_cap per family) in LDS, 4 bytes each: refuse what would not launch
    // (ck_create has refused it before it looked for a device)
    if ((size_t)ws.quad_cap * (size_t)cfg.n_families > (size_t)CK_MAX_FRAME_CANDIDATES) return CK_EINVAL;
    ws.det_cap = 256;
    ws.ht_size = next_pow2(2 * ws.cluster_cap);
    if (ws.ht_size < 1024) ws.ht_size = 1024;
    ws.max_cluster_points = 3 * (2 * h->qw + 2 * h->qh); // AprilTag-3's bound; <= 3 * 4 * 4095 < CK_HUGE_CAP (ck_create bounds the sides)
    if (cfg.max_nmaxima < 4 || cfg.max_nmaxima > 12) return CK_EINVAL;
    {   // frame pitch of the point arrays = positions of the split fit's extended sequences (ck_internal.h)
        size_t e = (size_t)ws.point_cap + (size_t)CK_EXT_HALO * ws.cluster_cap;
        e += (size_t)ck_ext_room(); // for CK_EXT_BASE (k_chunk.hip), the diagnostics library's shift of a frame's sequences: 0 in the product
        const size_t r = (e + CK_SPAN - 1) / CK_SPAN * CK_SPAN;
        if (r > 0x7FFFFFFFu - 4096) return CK_EINVAL;
        ws.ext_cap = (int)r;
    }
    ws.run_cap = 4 * ws.cluster_cap;
    ws.hcap = (ws.max_cluster_points + 1023) & ~1023;
    // fit scratch: one work list per size class + counters, then the decode candidates
    size_t list_bytes = ((size_t)CK_FIT_LISTS * ws.cluster_cap * nb + 32) * sizeof(uint32_t);
    size_t cand_bytes = 256 + ((nb * 4 + 255) / 256) * 256 + sizeof(ck_detection_t) * (size_t)ws.quad_cap * cfg.n_families * nb;
    ws.fit_scratch_bytes = ((list_bytes + 255) / 256) * 256 + cand_bytes;
    ws.field_cap = 1024;
    return CK_OK;
}

int ck_bufs_create(ck_handle *h) {
    int rc = stage_caps(h);
    for (const ck_buf_desc &d : ck_bufs) {
        const bool now = !(d.flags & CK_BUF_LAZY) || (d.member == offsetof(ck_handle, d_qframes) && h->cfg.quad_decimate > 1);
        if (rc == CK_OK && now) rc = alloc_one(h, d);
    }
    if (rc != CK_OK) return rc;
    // family tables: the codes go into d_fam_codes one family after the other
    const ck_config_t &cfg = h->cfg;
    std::vector<ck_dev_family> fams((size_t)cfg.n_families);
    uint64_t *dc = h->d_fam_codes;
    for (int f = 0; f < cfg.n_families; f++) {
        const ck_family_t *src = cfg.families[f];
        ck_dev_family &d = fams[(size_t)f];
        memset(&d, 0, sizeof d);
        d.nbits = src->nbits; d.ncodes = src->ncodes; d.n_upstream = src->n_upstream ? src->n_upstream : src->ncodes; /* 0 (a table built against ABI v1, or zero-initialised): the caller vouches for all of it */ d.width_at_border = src->width_at_border;
        d.total_width = src->total_width; d.reversed_border = src->reversed_border;
        for (uint32_t i = 0; i < src->nbits; i++) { d.bit_x[i] = src->bit_x[i]; d.bit_y[i] = src->bit_y[i]; }
        CK_HIP(hipMemcpy(dc, src->codes, sizeof(uint64_t) * src->ncodes, hipMemcpyHostToDevice));
        d.codes = dc;
        dc += src->ncodes;
    }
    CK_HIP(hipMemcpy(h->d_fams, fams.data(), sizeof(ck_dev_family) * fams.size(), hipMemcpyHostToDevice));
    return CK_OK;
}

// the whole detector on n frames resident on the device: threshold + segmentation -> clusters -> quad fit -> decode, all on
// h->stream (the quad fit alone puts some size classes on the handle's side streams: k_quads.hip)
static int run_pipeline(ck_handle *h, const ck_dev_image &img, int n, int upto /*1 clusters, 2 quads, 3 all*/) {
    hipEvent_t *ev = h->ev;
    h->n_last_dets = -1; // the workspace is rewritten from here on; it holds this call's detections only once they are all enqueued
    h->n_pose_inputs = -1;
    h->last_img_p = img.p; h->last_img_stride = img.stride; h->last_img_pitch = img.pitch;
    CK_HIP(hipEventRecord(ev[1], h->stream));
    int rc = ck_run_threshold_segment(h, img, n);
    if (rc != CK_OK) return rc;
    CK_HIP(hipEventRecord(ev[2], h->stream));
    rc = ck_launch_clusters(h, n);
    if (rc != CK_OK) return rc;
    CK_HIP(hipEventRecord(ev[3], h->stream));
    const ck_dev_image fine = ck_refine_image(h, img);
    if (upto >= 2) {
        rc = ck_launch_fit_quads(h, ck_quad_image(h, img), fine, n);
        if (rc != CK_OK) return rc;
    }
    CK_HIP(hipEventRecord(ev[4], h->stream));
    if (upto >= 3) {
        rc = ck_launch_decode(h, fine, n);
        if (rc == CK_OK) rc = ck_launch_subpix_dets(h, img, n); // ck_set_corner_subpix: on the unfiltered frame (nothing when off)
        if (rc != CK_OK) return rc;
    }
    CK_HIP(hipEventRecord(ev[5], h->stream));
    if (upto >= 3) h->n_last_dets = n;
    return CK_OK;
}

static void fill_stage_ms(ck_handle *h) {
    ck_stage_ms_t &ms = h->last_ms;
    float t;
    auto el = [&](int a, int b) { t = 0; (void)hipEventElapsedTime(&t, h->ev[a], h->ev[b]); return t; };
    ms.h2d = el(0, 1); ms.threshold = el(1, 2); ms.segment = 0; ms.clusters = el(2, 3); ms.quads = el(3, 4);
    ms.decode = el(4, 5); ms.d2h = el(5, 6); ms.total = el(0, 6); // (ck_process_*: d2h slot = glue + SQPnP + 64-byte records back)
}

static int fetch_detections(ck_handle *h, int n, ck_detection_t *dets, int cap, int32_t *counts, uint32_t *status) {
    ck_stage_ws &ws = h->ws;
    std::vector<uint32_t> counters((size_t)n * CK_CNT_STRIDE);
    std::vector<ck_detection_t> all((size_t)n * ws.det_cap);
    CK_HIP(hipMemcpyAsync(counters.data(), ws.d_counters, counters.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    CK_HIP(hipMemcpyAsync(all.data(), ws.d_dets, all.size() * sizeof(ck_detection_t), hipMemcpyDeviceToHost, h->stream));
    CK_HIP(hipEventRecord(h->ev[6], h->stream));
    CK_HIP(hipStreamSynchronize(h->stream));
    for (int i = 0; i < n; i++) {
        uint32_t nd = counters[(size_t)i * CK_CNT_STRIDE + CK_CNT_DETS];
        uint32_t st = counters[(size_t)i * CK_CNT_STRIDE + CK_CNT_STATUS];
        if ((int)nd > cap) { nd = (uint32_t)cap; st |= CK_FRAME_DETS_OVERFLOW; }
        memcpy(dets + (size_t)i * cap, all.data() + (size_t)i * ws.det_cap, sizeof(ck_detection_t) * nd);
        counts[i] = (int32_t)nd;
        if (status) status[i] = st;
    }
    fill_stage_ms(h);
    return CK_OK;
}

// what every detect entry point does once its input is staged (ev[0] recorded before the staging)
static int detect_common(ck_handle *h, const ck_dev_image &img, int n, ck_detection_t *dets, int cap, int32_t *counts, uint32_t *status) {
    const int rc = run_pipeline(h, img, n, 3);
    if (rc != CK_OK) return rc;
    return fetch_detections(h, n, dets, cap, counts, status);
}

extern "C" int ck_detect_uploaded(ck_handle_t *h, int32_t n, ck_detection_t *dets, int32_t cap, int32_t *counts, uint32_t *status) {
    if (!h || !dets || !counts || cap < 1 || n < 0 || n > h->n_staged) return CK_EINVAL;
    if (n == 0) return CK_OK;
    CK_HIP(hipSetDevice(h->device));
    CK_HIP(hipEventRecord(h->ev[0], h->stream));
    return detect_common(h, ck_staged_image(h), n, dets, cap, counts, status);
}

extern "C" int ck_detect_batch(ck_handle_t *h, const ck_image_u8_t *imgs, int32_t n, ck_detection_t *dets, int32_t cap,
                               int32_t *counts, uint32_t *status) {
    if (!h || !dets || !counts || cap < 1 || n < 0) return CK_EINVAL;
    if (n == 0) return CK_OK;
    CK_HIP(hipSetDevice(h->device));
    CK_HIP(hipEventRecord(h->ev[0], h->stream));
    int rc = ck_upload_frames(h, imgs, n);
    if (rc != CK_OK) return rc;
    return detect_common(h, ck_staged_image(h), n, dets, cap, counts, status);
}

extern "C" int ck_detect_batch_device(ck_handle_t *h, const uint8_t *d_frames, int32_t n, int32_t stride, int64_t frame_pitch,
                                      ck_detection_t *dets, int32_t cap, int32_t *counts, uint32_t *status) {
    if (!h || !dets || !counts || cap < 1 || n < 0) return CK_EINVAL;
    if (n == 0) return CK_OK;
    CK_HIP(hipSetDevice(h->device));
    CK_HIP(hipEventRecord(h->ev[0], h->stream));
    ck_dev_image use;
    int rc = ck_stage_device_frames(h, d_frames, n, stride, frame_pitch, &use);
    if (rc != CK_OK) return rc;
    return detect_common(h, use, n, dets, cap, counts, status);
}

int ck_detect_frames(ck_handle *h, const ck_dev_image &img, int n, ck_detection_t *dets, int cap, int32_t *counts, uint32_t *status) {
    if (!h || !dets || !counts || cap < 1 || n < 0 || n > h->cfg.max_batch) return CK_EINVAL;
    if (n == 0) return CK_OK;
    CK_HIP(hipEventRecord(h->ev[0], h->stream));
    return detect_common(h, img, n, dets, cap, counts, status);
}

// ck_clusters_batch / ck_quads_batch: stage the input, run up to stage `upto`, wait, read the frames' counters
static int run_upto(ck_handle *h, const ck_image_u8_t *imgs, int n, int upto, std::vector<uint32_t> &counters) {
    CK_HIP(hipSetDevice(h->device));
    int rc = imgs ? ck_upload_frames(h, imgs, n) : (n <= h->n_staged ? CK_OK : CK_EINVAL);
    if (rc != CK_OK) return rc;
    rc = run_pipeline(h, ck_staged_image(h), n, upto);
    if (rc != CK_OK) return rc;
    CK_HIP(hipStreamSynchronize(h->stream));
    counters.resize((size_t)n * CK_CNT_STRIDE);
    CK_HIP(hipMemcpy(counters.data(), h->ws.d_counters, counters.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return CK_OK;
}

extern "C" int ck_clusters_batch(ck_handle_t *h, const ck_image_u8_t *imgs, int32_t n, ck_cluster_t *clusters, int32_t cluster_cap,
                                 int32_t *n_clusters, ck_cluster_point_t *points, int32_t point_cap, int32_t *n_points) {
    if (!h || !clusters || !n_clusters || !points || !n_points || n < 0 || cluster_cap < 0 || point_cap < 0) return CK_EINVAL;
    if (n == 0) return CK_OK;
    std::vector<uint32_t> counters;
    int rc = run_upto(h, imgs, n, 1, counters);
    if (rc != CK_OK) return rc;
    ck_stage_ws &ws = h->ws;
    for (int i = 0; i < n; i++) {
        // On the device a twin point is one word and the records count words (ck_internal.h); the caller gets every point on its own:
        // a twin becomes its two points, and start / count / n_points are the logical ones, the records tiling the point array
        // in their own order as they do on the device.
        uint32_t nc = counters[(size_t)i * CK_CNT_STRIDE + CK_CNT_CLUSTERS], np = counters[(size_t)i * CK_CNT_STRIDE + CK_CNT_POINTS];
        if ((int)nc > cluster_cap) return CK_ECAPACITY;
        ck_cluster_t *cl = clusters + (size_t)i * cluster_cap;
        CK_HIP(hipMemcpy(cl, ws.d_clusters + (size_t)i * ws.cluster_cap, sizeof(ck_cluster_t) * nc, hipMemcpyDeviceToHost));
        std::vector<ck_packed_point> packed(np);
        CK_HIP(hipMemcpy(packed.data(), ws.d_points + (size_t)i * ws.ext_cap, sizeof(ck_packed_point) * np, hipMemcpyDeviceToHost));
        size_t total = np;
        for (uint32_t k = 0; k < np; k++) total += (packed[k] & CK_PT_TWIN) ? 1u : 0u;
        if (total > (size_t)point_cap) return CK_ECAPACITY;
        ck_cluster_point_t *out = points + (size_t)i * point_cap;
        uint32_t at = 0;
        for (uint32_t c = 0; c < nc; c++) {
            const uint32_t s0 = cl[c].start, s1 = cl[c].count ? s0 + cl[c].count : s0; // (an empty record: a cluster k_scan had no room for)
            if (s1 > np) return CK_EDEVICE; // (cannot happen: k_scan keeps a cluster only when its points fit)
            cl[c].start = cl[c].count ? at : 0u;
            for (uint32_t k = s0; k < s1; k++) {
                out[at++] = ck_unpack_point(packed[k]);
                if (packed[k] & CK_PT_TWIN) out[at++] = ck_unpack_twin(packed[k]);
            }
            cl[c].count = cl[c].count ? at - cl[c].start : 0u;
        }
        n_clusters[i] = (int32_t)nc; n_points[i] = (int32_t)at;
    }
    return CK_OK;
}

extern "C" int ck_quads_batch(ck_handle_t *h, const ck_image_u8_t *imgs, int32_t n, ck_quad_t *quads, int32_t quad_cap, int32_t *n_quads) {
    if (!h || !quads || !n_quads || n < 0 || quad_cap < 0) return CK_EINVAL;
    if (n == 0) return CK_OK;
    std::vector<uint32_t> counters;
    int rc = run_upto(h, imgs, n, 2, counters);
    if (rc != CK_OK) return rc;
    ck_stage_ws &ws = h->ws;
    for (int i = 0; i < n; i++) {
        uint32_t nq = counters[(size_t)i * CK_CNT_STRIDE + CK_CNT_QUADS];
        if (nq > (uint32_t)ws.quad_cap) nq = (uint32_t)ws.quad_cap; // the counter keeps counting past the capacity (status bit set)
        if ((int)nq > quad_cap) return CK_ECAPACITY;
        CK_HIP(hipMemcpy(quads + (size_t)i * quad_cap, ws.d_quads + (size_t)i * ws.quad_cap, sizeof(ck_quad_t) * nq, hipMemcpyDeviceToHost));
        n_quads[i] = (int32_t)nq;
    }
    return CK_OK;
}

// ck_launch_decode on the caller's quads: the frames' counters and candidate counts are written from the host (quad count set,
// everything else zero: the status word can only carry what decode sets), the quads copied into d_quads
extern "C" int ck_decode_quads_batch(ck_handle_t *h, const ck_image_u8_t *imgs, int32_t n, const ck_quad_t *quads, int32_t quad_stride,
                                     const int32_t *n_quads, ck_detection_t *dets, int32_t cap, int32_t *counts, uint32_t *status) {
    if (!h || !quads || !n_quads || !dets || !counts || cap < 1 || n < 0 || quad_stride < 0) return CK_EINVAL;
    if (!imgs && n > h->n_staged) return CK_EINVAL;
    if (n > h->cfg.max_batch) return imgs ? CK_ECAPACITY : CK_EINVAL;
    ck_stage_ws &ws = h->ws;
    for (int i = 0; i < n; i++)
        if (n_quads[i] < 0 || n_quads[i] > quad_stride || n_quads[i] > ws.quad_cap) return CK_EINVAL;
    if (n == 0) return CK_OK;
    CK_HIP(hipSetDevice(h->device));
    CK_HIP(hipEventRecord(h->ev[0], h->stream));
    if (imgs) {
        int rc = ck_upload_frames(h, imgs, n);
        if (rc != CK_OK) return rc;
    }
    h->n_last_dets = -1;
    h->n_pose_inputs = -1;
    const ck_dev_image staged = ck_staged_image(h);
    CK_HIP(hipEventRecord(h->ev[1], h->stream));
    if (ck_refine_reads_quad(h)) { // decode reads the filtered frame: make it
        int rc = ck_make_quad_image(h, staged, n);
        if (rc != CK_OK) return rc;
    }
    for (int e = 2; e <= 4; e++) CK_HIP(hipEventRecord(h->ev[e], h->stream));
    // the copies below read the caller's quads and this vector while they are in flight: no return before the stream has drained
    std::vector<uint32_t> counters((size_t)n * CK_CNT_STRIDE, 0u);
    auto enqueue = [&]() -> int {
        for (int i = 0; i < n; i++) {
            counters[(size_t)i * CK_CNT_STRIDE + CK_CNT_QUADS] = (uint32_t)n_quads[i];
            if (n_quads[i])
                CK_HIP(hipMemcpyAsync(ws.d_quads + (size_t)i * ws.quad_cap, quads + (size_t)i * quad_stride, sizeof(ck_quad_t) * (size_t)n_quads[i],
                                      hipMemcpyHostToDevice, h->stream));
        }
        CK_HIP(hipMemcpyAsync(ws.d_counters, counters.data(), counters.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
        CK_HIP(hipMemsetAsync(ck_fit_scratch_layout(ws, h->cfg.max_batch).cand_count, 0, sizeof(uint32_t) * (size_t)n, h->stream));
        int rc = ck_launch_decode(h, ck_refine_image(h, staged), n);
        if (rc != CK_OK) return rc;
        CK_HIP(hipEventRecord(h->ev[5], h->stream));
        return CK_OK;
    };
    int rc = enqueue();
    if (rc != CK_OK) { (void)hipStreamSynchronize(h->stream); return rc; }
    return fetch_detections(h, n, dets, cap, counts, status);
}

static int process_common(ck_handle *h, const ck_dev_image &img, int n, const ck_process_params_t *pp, const double *gyro,
                          const uint8_t *has_gyro, ck_vision_measurement_t *out, int32_t *valid) {
    if (!pp || !gyro || !has_gyro || !out || !valid || (pp->n_field > 0 && !pp->field) || pp->n_field < 0) return CK_EINVAL;
    CK_HIP(hipEventRecord(h->ev[0], h->stream));
    if (pp->n_field > h->ws.field_cap) return CK_ECAPACITY;
    if (pp->n_field) CK_HIP(hipMemcpyAsync(h->ws.d_field, pp->field, sizeof(ck_field_tag_t) * (size_t)pp->n_field, hipMemcpyDefault, h->stream));
    int rc = run_pipeline(h, img, n, 3);
    if (rc != CK_OK) return rc;
    rc = ck_run_pose(h, n, pp, gyro, has_gyro, out, valid, false, false);
    h->n_last_pose = rc == CK_OK ? n : -1;
    h->n_pose_inputs = h->n_last_pose;
    CK_HIP(hipEventRecord(h->ev[6], h->stream));
    CK_HIP(hipStreamSynchronize(h->stream));
    fill_stage_ms(h);
    return rc;
}

int ck_process_frames(ck_handle *h, const ck_dev_image &img, int n, const ck_process_params_t *pp, const double *gyro,
                      const uint8_t *has_gyro, ck_vision_measurement_t *out, int32_t *valid) {
    if (!h || n < 0 || n > h->cfg.max_batch) return CK_EINVAL;
    if (n == 0) return CK_OK;
    return process_common(h, img, n, pp, gyro, has_gyro, out, valid);
}

extern "C" int ck_process_uploaded(ck_handle_t *h, int32_t n, const ck_process_params_t *pp, const double *gyro, const uint8_t *has_gyro,
                                   ck_vision_measurement_t *out, int32_t *valid) {
    if (!h || n < 0 || n > h->n_staged) return CK_EINVAL;
    if (n == 0) return CK_OK;
    CK_HIP(hipSetDevice(h->device));
    return process_common(h, ck_staged_image(h), n, pp, gyro, has_gyro, out, valid);
}

extern "C" int ck_process_batch_device(ck_handle_t *h, const uint8_t *d_frames, int32_t n, int32_t stride, int64_t frame_pitch,
                                       const ck_process_params_t *pp, const double *gyro, const uint8_t *has_gyro,
                                       ck_vision_measurement_t *out, int32_t *valid) {
    if (!h) return CK_EINVAL;
    if (n == 0) return CK_OK;
    CK_HIP(hipSetDevice(h->device));
    ck_dev_image use;
    int rc = ck_stage_device_frames(h, d_frames, n, stride, frame_pitch, &use);
    if (rc != CK_OK) return rc;
    return process_common(h, use, n, pp, gyro, has_gyro, out, valid);
}
