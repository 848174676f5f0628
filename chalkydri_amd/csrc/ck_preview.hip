// JPEG preview of the staged frames: the host half.  Resolves the geometry (ck_preview_layout: the one place),
// builds the quantisation divisors and the file header of a call, grows the workspace and enqueues the stages of k_jpegenc.hip on
// the handle's stream; only the sizes and the bytes used come back to a host buffer.
#include <new>
#include <string.h>

#include "ck_preview.h"

namespace {

// ITU-T T.81 Annex K.1, luminance, natural order
const uint8_t kStdQ[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
                           14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                           49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                              41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                              30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// Annex K.3 luminance tables as a DHT segment carries them: codes per length, then the symbols
const uint8_t kDcBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
const uint8_t kAcBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
const uint8_t kAcVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
    0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
    0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
    0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

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
    memcpy(p, kDcBits, 16); p += 16;
    for (int k = 0; k < 12; k++) *p++ = (uint8_t)k;
    seg(0xC4, 179);
    *p++ = 0x10;
    memcpy(p, kAcBits, 16); p += 16;
    memcpy(p, kAcVals, 162); p += 162;
    if (pp->restart_rows) {
        seg(0xDD, 2);
        *p++ = (uint8_t)(g.R >> 8); *p++ = (uint8_t)(g.R & 255);
    }
    seg(0xDA, 6);
    *p++ = 1; *p++ = 1; *p++ = 0x00; *p++ = 0; *p++ = 63; *p++ = 0;
}

template <typename T>
int grow_dev(T **p, size_t *cap, size_t need) { // capacities in bytes
    if (need <= *cap) return CK_OK;
    (void)ck_free_dev(*p);
    *p = nullptr; *cap = 0;
    const size_t want = need + need / 4;
    CK_HIP_ALLOC(ck_malloc_dev(p, want));
    *cap = want;
    return CK_OK;
}

template <typename T>
int grow_host(T **p, size_t *cap, size_t need) {
    if (need <= *cap) return CK_OK;
    if (*p) (void)hipHostFree(*p);
    *p = nullptr; *cap = 0;
    const size_t want = need + need / 4;
    if (hipHostMalloc(reinterpret_cast<void **>(p), want, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
        return CK_ENOMEM;
    }
    *cap = want;
    return CK_OK;
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
    for (int i = 0; i < n; i++) {
        const int f = frames ? frames[i] : i;
        if (f < 0 || f >= h->n_staged) return CK_EINVAL;
        if (pg->overlay && f >= h->n_last_dets) return CK_EINVAL;
    }
    if (n == 0) return CK_OK;
    CK_HIP(hipSetDevice(h->device));
    if (!h->preview) {
        h->preview = new (std::nothrow) ck_preview_ws();
        if (!h->preview) return CK_ENOMEM;
        memset(h->preview, 0, sizeof *h->preview);
    }
    ck_preview_ws &P = *h->preview;
    rc = grow_dev(&P.d_frames, &P.frames_cap, sizeof(int32_t) * (size_t)n);
    if (rc == CK_OK) rc = grow_host(&P.h_sizes, &P.h_sizes_cap, sizeof(int64_t) * 4 * (size_t)n);
    if (rc == CK_OK && pg->overlay) rc = grow_dev(&P.d_mask, &P.mask_cap, sizeof(uint32_t) * (size_t)pg->mask_words * n);
    if (rc != CK_OK) return rc;
    int32_t *idx = reinterpret_cast<int32_t *>(P.h_sizes + 3 * (size_t)n); // (pinned; every call ends with a synchronisation)
    for (int i = 0; i < n; i++) idx[i] = frames ? frames[i] : i;
    CK_HIP(hipMemcpyAsync(P.d_frames, idx, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, h->stream));
    return ck_launch_preview_mask(h, *pg, n);
}

} // namespace

static_assert(sizeof(ck_preview_params_t) == 24, "ck_preview_params_t layout");

void ck_preview_free(ck_handle *h) {
    if (!h || !h->preview) return;
    ck_preview_ws &P = *h->preview;
    if (P.h_sizes) (void)hipHostFree(P.h_sizes);
    if (P.h_out) (void)hipHostFree(P.h_out);
    (void)ck_free_dev(P.d_frames); (void)ck_free_dev(P.d_mask); (void)ck_free_dev(P.d_coef); (void)ck_free_dev(P.d_dc);
    (void)ck_free_dev(P.d_len); (void)ck_free_dev(P.d_istart); (void)ck_free_dev(P.d_bits); (void)ck_free_dev(P.d_cpre);
    (void)ck_free_dev(P.d_sizes); (void)ck_free_dev(P.d_out);
    delete h->preview;
    h->preview = nullptr;
}

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
    rc = grow_dev(&P.d_out, &P.out_cap, bytes);
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
    rc = grow_dev(&P.d_coef, &P.coef_cap, sizeof(int16_t) * 64 * nb);
    if (rc == CK_OK) rc = grow_dev(&P.d_dc, &P.dc_cap, sizeof(int16_t) * nb);
    if (rc == CK_OK) rc = grow_dev(&P.d_len, &P.len_cap, sizeof(uint32_t) * nb);
    if (rc == CK_OK) rc = grow_dev(&P.d_istart, &P.istart_cap, sizeof(uint32_t) * (size_t)(g.nint + 1) * n);
    if (rc == CK_OK) rc = grow_dev(&P.d_bits, &P.bits_cap, sizeof(uint32_t) * (size_t)g.bit_words * n);
    if (rc == CK_OK) rc = grow_dev(&P.d_cpre, &P.cpre_cap, sizeof(uint32_t) * (size_t)g.chunk_cap * n);
    if (rc == CK_OK) rc = grow_dev(&P.d_sizes, &P.sizes_cap, sizeof(int64_t) * 3 * (size_t)n);
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
        rc = grow_dev(&P.d_out, &P.out_cap, total);
        if (rc == CK_OK) rc = grow_host(&P.h_out, &P.h_out_cap, total);
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
