// JPEG preview of the staged frames: the host half.  Resolves the geometry (ck_preview_layout: the one place),
// builds the quantisation divisors and the file header of a call, grows the workspace and enqueues the stages of k_jpegenc.hip on
// the handle's stream; only the sizes and the bytes used come back to a host buffer.
#include <string.h>

#include "ck_jpeg_tables.h"
#include "ck_preview.h"

namespace {

// SOI 2, APP0 18, DQT 69, SOF0 13, DHT DC 33, DHT AC 183, DRI 6 (only with a restart interval), SOS 10
int header_len(int restart_rows) { return 2 + 18 + 69 + 13 + 33 + 183 + (restart_rows ? 6 : 0) + 10; }

// geometry of a call; CK_EINVAL as ck_preview_layout documents it
int resolve(const ck_preview_params_t *pp, int W, int H, ck_pv_geom *g) {
    if (!pp || W < 1 || H < 1 || pp->width < 0 || pp->height < 0) return CK_EINVAL;
    if (pp->quality < 1 || pp->quality > 100 || pp->restart_rows < 0) return CK_EINVAL;
    if (pp->overlay != 0 && pp->overlay != 1) return CK_EINVAL;
    memset(g, 0, sizeof *g);
    g->W = W; g->H = H;
    g->pw = pp->width == 0 || pp->width > W ? W : pp->width;
    g->ph = pp->height == 0 || pp->height > H ? H : pp->height;
    if (g->pw < 8 || g->ph < 8) return CK_EINVAL;
    g->bw = (g->pw + 7) / 8; g->bh = (g->ph + 7) / 8; g->nblk = g->bw * g->bh;
    if ((int64_t)pp->restart_rows * g->bw > 65535) return CK_EINVAL;
    g->R = pp->restart_rows ? pp->restart_rows * g->bw : g->nblk;
    g->nint = (g->nblk + g->R - 1) / g->R;
    g->overlay = pp->overlay;
    g->mask_words = (int)(((int64_t)g->pw * g->ph + 31) / 32);
    const int64_t max_scan = (int64_t)g->nblk * CK_PV_BLOCK_BYTES + g->nint; // every interval rounds up to a whole byte
    g->chunk_cap = (int)((max_scan + CK_PV_CHUNK - 1) / CK_PV_CHUNK) + 1;
    g->bit_words = g->chunk_cap * (CK_PV_CHUNK / 4);
    g->hdr_len = header_len(pp->restart_rows);
    return CK_OK;
}

int64_t max_file_bytes(const ck_pv_geom &g) { // every byte of the scan stuffed, markers, header, EOI
    return g.hdr_len + 2 * ((int64_t)g.nblk * CK_PV_BLOCK_BYTES + g.nint) + 2 * (int64_t)(g.nint - 1) + 2;
}

// libjpeg's jpeg_set_quality(quality, force_baseline) on the K.1 table; the header as libjpeg writes it for one component
void make_tables(const ck_preview_params_t *pp, const ck_pv_geom &g, ck_pv_tables *t) {
    memset(t, 0, sizeof *t);
    const int q = pp->quality, scale = q < 50 ? 5000 / q : 200 - 2 * q;
    uint8_t qt[64];
    for (int k = 0; k < 64; k++) {
        int v = (kStdQ[k] * scale + 50) / 100;
        v = v < 1 ? 1 : (v > 255 ? 255 : v);
        qt[k] = (uint8_t)v;
        t->qdiv[k] = (uint16_t)(8 * v);
    }
    uint8_t *p = t->hdr;
    auto seg = [&](int marker, int body) { *p++ = 0xFF; *p++ = (uint8_t)marker; *p++ = (uint8_t)((body + 2) >> 8); *p++ = (uint8_t)((body + 2) & 255); };
    *p++ = 0xFF; *p++ = 0xD8;
    seg(0xE0, 14);
    const uint8_t jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0}; // 1.01, no units, density 1 x 1, no thumbnail
    memcpy(p, jfif, 14); p += 14;
    seg(0xDB, 65);
    *p++ = 0; // 8-bit, table 0
    for (int k = 0; k < 64; k++) *p++ = qt[kNatural[k]];
    seg(0xC0, 9);
    *p++ = 8; *p++ = (uint8_t)(g.ph >> 8); *p++ = (uint8_t)(g.ph & 255); *p++ = (uint8_t)(g.pw >> 8); *p++ = (uint8_t)(g.pw & 255);
    *p++ = 1; *p++ = 1; *p++ = 0x11; *p++ = 0;
    seg(0xC4, 29);
    *p++ = 0x00;
    memcpy(p, kStdHuff[0][0].bits, 16); p += 16;
    memcpy(p, kStdHuff[0][0].vals, 12); p += 12;
    seg(0xC4, 179);
    *p++ = 0x10;
    memcpy(p, kStdHuff[1][0].bits, 16); p += 16;
    memcpy(p, kStdHuff[1][0].vals, 162); p += 162;
    if (pp->restart_rows) {
        seg(0xDD, 2);
        *p++ = (uint8_t)(g.R >> 8); *p++ = (uint8_t)(g.R & 255);
    }
    seg(0xDA, 6);
    *p++ = 1; *p++ = 1; *p++ = 0x00; *p++ = 0; *p++ = 63; *p++ = 0;
}

bool is_device_pointer(const void *p) {
    hipPointerAttribute_t a;
    memset(&a, 0, sizeof a);
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError(); // (plain host memory the runtime has never seen)
        return false;
    }
    return a.type == hipMemoryTypeDevice;
}

// what every entry point checks, in the contract's order; then the index list on the device.  *pg is the call's geometry.
int begin(ck_handle *h, const ck_preview_params_t *pp, const int32_t *frames, int32_t n, const void *out, ck_pv_geom *pg) {
    if (!h || !pp || !out || n < 0) return CK_EINVAL;
    int rc = resolve(pp, h->w, h->h, pg);
    if (rc != CK_OK) return rc;
    if (n > h->cfg.max_batch) return CK_ECAPACITY;
    // the overlay reads the detections of the last detect / process call: ck_last_tag_poses' rule
    if (pg->overlay && h->n_last_dets < 1) return CK_EINVAL;
    if (!ck_frame_list_ok(frames, n, h->n_staged) || (pg->overlay && !ck_frame_list_ok(frames, n, h->n_last_dets))) return CK_EINVAL;
    if (n == 0) return CK_OK;
    CK_HIP(hipSetDevice(h->device));
    if (!ck_workspace(h->preview)) return CK_ENOMEM;
    ck_preview_ws &P = *h->preview;
    rc = P.d_frames.reserve(sizeof(int32_t) * (size_t)n);
    if (rc == CK_OK) rc = P.h_sizes.reserve(sizeof(int64_t) * 4 * (size_t)n);
    if (rc == CK_OK && pg->overlay) rc = P.d_mask.reserve(sizeof(uint32_t) * (size_t)pg->mask_words * n);
    if (rc != CK_OK) return rc;
    int32_t *idx = reinterpret_cast<int32_t *>(P.h_sizes + 3 * (size_t)n); // (pinned; every call ends with a synchronisation)
    for (int i = 0; i < n; i++) idx[i] = frames ? frames[i] : i;
    CK_HIP(hipMemcpyAsync(P.d_frames, idx, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, h->stream));
    return ck_launch_preview_mask(h, *pg, n);
}

} // namespace

static_assert(sizeof(ck_preview_params_t) == 24, "ck_preview_params_t layout");

extern "C" void ck_preview_params_default(ck_preview_params_t *pp) {
    if (!pp) return;
    memset(pp, 0, sizeof *pp);
    pp->width = 640; pp->height = 480; // the caps filter of the reference's stream (mjpeg.rs:41-49)
    pp->quality = 50;                  // turbojpeg::compress(.., 50, ..) (mjpeg.rs:116)
}

extern "C" int ck_preview_layout(const ck_preview_params_t *pp, int32_t W, int32_t H, int32_t *pw, int32_t *ph, int64_t *max_bytes) {
    ck_pv_geom g;
    const int rc = resolve(pp, W, H, &g);
    if (rc != CK_OK) return rc;
    if (pw) *pw = g.pw;
    if (ph) *ph = g.ph;
    if (max_bytes) *max_bytes = max_file_bytes(g);
    return CK_OK;
}

extern "C" int ck_preview_luma(ck_handle_t *h, const ck_preview_params_t *pp, const int32_t *frames, int32_t n, uint8_t *out) {
    ck_pv_geom g;
    int rc = begin(h, pp, frames, n, out, &g);
    if (rc != CK_OK || n == 0) return rc;
    ck_preview_ws &P = *h->preview;
    const size_t bytes = (size_t)g.pw * g.ph * n;
    rc = P.d_out.reserve(bytes);
    if (rc == CK_OK) rc = ck_launch_preview_luma(h, g, n, P.d_out);
    if (rc != CK_OK) return rc;
    CK_HIP(hipMemcpyAsync(out, P.d_out, bytes, hipMemcpyDefault, h->stream));
    CK_HIP(hipStreamSynchronize(h->stream));
    return CK_OK;
}

extern "C" int ck_preview_jpeg(ck_handle_t *h, const ck_preview_params_t *pp, const int32_t *frames, int32_t n, uint8_t *out,
                               int64_t cap_per_frame, int64_t *sizes, uint32_t *status) {
    if (!sizes || cap_per_frame < 1) return CK_EINVAL;
    ck_pv_geom g;
    int rc = begin(h, pp, frames, n, out, &g);
    if (rc != CK_OK || n == 0) return rc;
    ck_preview_ws &P = *h->preview;
    ck_pv_tables tab;
    make_tables(pp, g, &tab);
    const size_t nb = (size_t)g.nblk * n;
    rc = P.d_coef.reserve(sizeof(int16_t) * 64 * nb);
    if (rc == CK_OK) rc = P.d_dc.reserve(sizeof(int16_t) * nb);
    if (rc == CK_OK) rc = P.d_len.reserve(sizeof(uint32_t) * nb);
    if (rc == CK_OK) rc = P.d_istart.reserve(sizeof(uint32_t) * (size_t)(g.nint + 1) * n);
    if (rc == CK_OK) rc = P.d_bits.reserve(sizeof(uint32_t) * (size_t)g.bit_words * n);
    if (rc == CK_OK) rc = P.d_cpre.reserve(sizeof(uint32_t) * (size_t)g.chunk_cap * n);
    if (rc == CK_OK) rc = P.d_sizes.reserve(sizeof(int64_t) * 3 * (size_t)n);
    if (rc != CK_OK) return rc;
    const bool direct = is_device_pointer(out); // a caller's device buffer is written in place: file i at out + i * cap_per_frame
    rc = ck_launch_preview_encode(h, g, tab, n, nullptr, cap_per_frame, !direct);
    if (rc != CK_OK) return rc;
    // sizes first: they say how much staging the files need and how many bytes cross the bus
    CK_HIP(hipMemcpyAsync(P.h_sizes, P.d_sizes, sizeof(int64_t) * 3 * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    CK_HIP(hipStreamSynchronize(h->stream));
    const int64_t *hs = P.h_sizes, *off = P.h_sizes + n;
    const auto used = [&](int i) { return hs[i] < cap_per_frame ? hs[i] : cap_per_frame; };
    const size_t total = (size_t)(off[n - 1] + used(n - 1));
    if (!direct) {
        rc = P.d_out.reserve(total);
        if (rc == CK_OK) rc = P.h_out.reserve(total);
        if (rc != CK_OK) return rc;
    }
    rc = ck_launch_preview_encode(h, g, tab, n, direct ? out : P.d_out, cap_per_frame, !direct);
    if (rc != CK_OK) return rc;
    if (!direct) CK_HIP(hipMemcpyAsync(P.h_out, P.d_out, total, hipMemcpyDeviceToHost, h->stream));
    uint32_t *st = reinterpret_cast<uint32_t *>(P.h_sizes + 3 * (size_t)n);
    for (int i = 0; i < n; i++) st[i] = (uint32_t)P.h_sizes[2 * (size_t)n + i];
    CK_HIP(hipMemcpyAsync(sizes, P.h_sizes, sizeof(int64_t) * (size_t)n, hipMemcpyDefault, h->stream));
    if (status) CK_HIP(hipMemcpyAsync(status, st, sizeof(uint32_t) * (size_t)n, hipMemcpyDefault, h->stream));
    CK_HIP(hipStreamSynchronize(h->stream));
    if (!direct)
        for (int i = 0; i < n; i++) memcpy(out + (size_t)i * cap_per_frame, P.h_out + off[i], (size_t)used(i));
    return CK_OK;
}
