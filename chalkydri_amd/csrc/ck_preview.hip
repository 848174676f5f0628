// JPEG preview of the staged frames and of the raw colour frames behind them (§4g): the host half.  Resolves the
// geometry (ck_preview_layout: the one place), builds the quantisation divisors and the file header of a call, grows the workspace
// and enqueues the stages of k_jpegenc.hip on the handle's stream; only the sizes and the bytes used come back to a host buffer.
#include <string.h>

#include "ck_jpeg_tables.h"
#include "ck_preview.h"
#include "ck_raw_planes.h"
#include "ck_rawfmt.h"

namespace {

// SOI 2, APP0 18, DQT 69, SOF0 13, DHT DC 33, DHT AC 183, DRI 6 (only with a restart interval), SOS 10; with three components
// a second DQT and DHT pair and 2 bytes per further component in SOF0 (3 each) and SOS (2 each)
int header_len(int restart_rows, int nc) {
    return 2 + 18 + 69 + 13 + 33 + 183 + (restart_rows ? 6 : 0) + 10 + (nc == 3 ? 69 + 33 + 183 + 2 * 3 + 2 * 2 : 0);
}

// geometry of a call of nc components; CK_EINVAL as ck_preview_layout documents it
int resolve(const ck_preview_params_t *pp, int W, int H, int nc, ck_pv_geom *g) {
    if (!pp || W < 1 || H < 1 || pp->width < 0 || pp->height < 0) return CK_EINVAL;
    if (pp->quality < 1 || pp->quality > 100 || pp->restart_rows < 0) return CK_EINVAL;
    if (pp->overlay != 0 && pp->overlay != 1) return CK_EINVAL;
    memset(g, 0, sizeof *g);
    g->W = W; g->H = H;
    g->pw = pp->width == 0 || pp->width > W ? W : pp->width;
    g->ph = pp->height == 0 || pp->height > H ? H : pp->height;
    if (g->pw < 8 || g->ph < 8) return CK_EINVAL;
    g->nc = nc;
    g->bw = (g->pw + 7) / 8; g->bh = (g->ph + 7) / 8; g->nblk = nc * g->bw * g->bh;
    if ((int64_t)pp->restart_rows * g->bw > 65535) return CK_EINVAL;
    g->R = pp->restart_rows ? nc * pp->restart_rows * g->bw : g->nblk;
    g->nint = (g->nblk + g->R - 1) / g->R;
    g->overlay = pp->overlay;
    g->mask_words = (int)(((int64_t)g->pw * g->ph + 31) / 32);
    const int64_t max_scan = (int64_t)g->nblk * CK_PV_BLOCK_BYTES + g->nint; // every interval rounds up to a whole byte
    g->chunk_cap = (int)((max_scan + CK_PV_CHUNK - 1) / CK_PV_CHUNK) + 1;
    g->bit_words = g->chunk_cap * (CK_PV_CHUNK / 4);
    g->hdr_len = header_len(pp->restart_rows, nc);
    return CK_OK;
}

int64_t max_file_bytes(const ck_pv_geom &g) { // every byte of the scan stuffed, markers, header, EOI
    return g.hdr_len + 2 * ((int64_t)g.nblk * CK_PV_BLOCK_BYTES + g.nint) + 2 * (int64_t)(g.nint - 1) + 2;
}

// libjpeg's jpeg_set_quality(quality, force_baseline) on the K.1 tables; the header as libjpeg writes it for g.nc components
void make_tables(const ck_preview_params_t *pp, const ck_pv_geom &g, ck_pv_tables *t) {
    memset(t, 0, sizeof *t);
    const int q = pp->quality, scale = q < 50 ? 5000 / q : 200 - 2 * q, nc = g.nc, ntab = nc == 3 ? 2 : 1;
    uint8_t qt[2][64];
    for (int c = 0; c < 2; c++)
        for (int k = 0; k < 64; k++) {
            int v = ((c ? kStdQChroma[k] : kStdQ[k]) * scale + 50) / 100;
            v = v < 1 ? 1 : (v > 255 ? 255 : v);
            qt[c][k] = (uint8_t)v;
            t->qdiv[c][k] = (uint16_t)(8 * v);
        }
    uint8_t *p = t->hdr;
    auto seg = [&](int marker, int body) { *p++ = 0xFF; *p++ = (uint8_t)marker; *p++ = (uint8_t)((body + 2) >> 8); *p++ = (uint8_t)((body + 2) & 255); };
    *p++ = 0xFF; *p++ = 0xD8;
    seg(0xE0, 14);
    const uint8_t jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0}; // 1.01, no units, density 1 x 1, no thumbnail
    memcpy(p, jfif, 14); p += 14;
    for (int c = 0; c < ntab; c++) {
        seg(0xDB, 65);
        *p++ = (uint8_t)c; // 8-bit, table c
        for (int k = 0; k < 64; k++) *p++ = qt[c][kNatural[k]];
    }
    seg(0xC0, 6 + 3 * nc);
    *p++ = 8; *p++ = (uint8_t)(g.ph >> 8); *p++ = (uint8_t)(g.ph & 255); *p++ = (uint8_t)(g.pw >> 8); *p++ = (uint8_t)(g.pw & 255);
    *p++ = (uint8_t)nc;
    for (int c = 0; c < nc; c++) { *p++ = (uint8_t)(c + 1); *p++ = 0x11; *p++ = c ? 1 : 0; } // id, 1 x 1, Tq
    for (int c = 0; c < ntab; c++) {
        seg(0xC4, 29);
        *p++ = (uint8_t)c;
        memcpy(p, kStdHuff[0][c].bits, 16); p += 16;
        memcpy(p, kStdHuff[0][c].vals, 12); p += 12;
        seg(0xC4, 179);
        *p++ = (uint8_t)(0x10 | c);
        memcpy(p, kStdHuff[1][c].bits, 16); p += 16;
        memcpy(p, kStdHuff[1][c].vals, 162); p += 162;
    }
    if (pp->restart_rows) {
        seg(0xDD, 2);
        const int mcus = g.R / nc;
        *p++ = (uint8_t)(mcus >> 8); *p++ = (uint8_t)(mcus & 255);
    }
    seg(0xDA, 4 + 2 * nc);
    *p++ = (uint8_t)nc;
    for (int c = 0; c < nc; c++) { *p++ = (uint8_t)(c + 1); *p++ = c ? 0x11 : 0x00; } // id, Td | Ta
    *p++ = 0; *p++ = 63; *p++ = 0;
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

// what every entry point checks once its geometry *pg is resolved, in the contract's order; then the index list on the device.
// n_avail: the frames an index may name (the staged ones, or the raw frames of a colour call)
int begin(ck_handle *h, const int32_t *frames, int32_t n, int n_avail, const ck_pv_geom *pg) {
    if (n > h->cfg.max_batch) return CK_ECAPACITY;
    // the overlay reads the detections of the last detect / process call: ck_last_tag_poses' rule
    if (pg->overlay && h->n_last_dets < 1) return CK_EINVAL;
    if (!ck_frame_list_ok(frames, n, n_avail) || (pg->overlay && !ck_frame_list_ok(frames, n, h->n_last_dets))) return CK_EINVAL;
    if (n == 0) return CK_OK;
    CK_HIP(hipSetDevice(h->device));
    if (!ck_workspace(h->preview)) return CK_ENOMEM;
    ck_preview_ws &P = *h->preview;
    int rc = P.d_frames.reserve(sizeof(int32_t) * (size_t)n);
    if (rc == CK_OK) rc = P.h_sizes.reserve(sizeof(int64_t) * 4 * (size_t)n);
    if (rc == CK_OK && pg->overlay) rc = P.d_mask.reserve(sizeof(uint32_t) * (size_t)pg->mask_words * n);
    if (rc != CK_OK) return rc;
    int32_t *idx = reinterpret_cast<int32_t *>(P.h_sizes + 3 * (size_t)n); // (pinned; every call ends with a synchronisation)
    for (int i = 0; i < n; i++) idx[i] = frames ? frames[i] : i;
    CK_HIP(hipMemcpyAsync(P.d_frames, idx, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, h->stream));
    return ck_launch_preview_mask(h, *pg, n);
}
// the grey entry points: the staged frames
int begin(ck_handle *h, const ck_preview_params_t *pp, const int32_t *frames, int32_t n, const void *out, ck_pv_geom *pg) {
    if (!h || !pp || !out || n < 0) return CK_EINVAL;
    const int rc = resolve(pp, h->w, h->h, 1, pg);
    return rc != CK_OK ? rc : begin(h, frames, n, h->n_staged, pg);
}

// The files of a call whose index list and mask are on the device: both halves of k_jpegenc.hip around the copy of the sizes.
int encode_files(ck_handle *h, const ck_preview_params_t *pp, const ck_pv_geom &g, const ck_pv_src *cs, int n, uint8_t *out,
                 int64_t cap_per_frame, int64_t *sizes, uint32_t *status) {
    ck_preview_ws &P = *h->preview;
    ck_pv_tables tab;
    make_tables(pp, g, &tab);
    const size_t nb = (size_t)g.nblk * n;
    int rc = P.d_coef.reserve(sizeof(int16_t) * 64 * nb);
    if (rc == CK_OK) rc = P.d_dc.reserve(sizeof(int16_t) * nb);
    if (rc == CK_OK) rc = P.d_len.reserve(sizeof(uint32_t) * nb);
    if (rc == CK_OK) rc = P.d_istart.reserve(sizeof(uint32_t) * (size_t)(g.nint + 1) * n);
    if (rc == CK_OK) rc = P.d_bits.reserve(sizeof(uint32_t) * (size_t)g.bit_words * n);
    if (rc == CK_OK) rc = P.d_cpre.reserve(sizeof(uint32_t) * (size_t)g.chunk_cap * n);
    if (rc == CK_OK) rc = P.d_sizes.reserve(sizeof(int64_t) * 3 * (size_t)n);
    if (rc != CK_OK) return rc;
    const bool direct = is_device_pointer(out); // a caller's device buffer is written in place: file i at out + i * cap_per_frame
    rc = ck_launch_preview_encode(h, g, tab, cs, n, nullptr, cap_per_frame, !direct);
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
    rc = ck_launch_preview_encode(h, g, tab, cs, n, direct ? out : P.d_out, cap_per_frame, !direct);
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

// the pixels of a call, [bytes] of them, through the workspace's staging to a host or device `out`
template <typename Launch>
int read_pixels(ck_handle *h, size_t bytes, uint8_t *out, Launch launch) {
    ck_preview_ws &P = *h->preview;
    int rc = P.d_out.reserve(bytes);
    if (rc == CK_OK) rc = launch(P.d_out);
    if (rc != CK_OK) return rc;
    CK_HIP(hipMemcpyAsync(out, P.d_out, bytes, hipMemcpyDefault, h->stream));
    CK_HIP(hipStreamSynchronize(h->stream));
    return CK_OK;
}

// libjpeg's rgb_ycc_convert (jccolor.c) in 16-bit fixed point; row c = the weights of R, G, B in component c
constexpr int kYcc[3][3] = {{(int)CK_LUMA_R, (int)CK_LUMA_G, (int)CK_LUMA_B}, {-11059, -21709, 32768}, {32768, -27439, -5329}};
constexpr int kYccBias[3] = {32768, (128 << 16) + 32767, (128 << 16) + 32767};

int overlay_component(int c) { return (kYcc[c][0] * 0 + kYcc[c][1] * 255 + kYcc[c][2] * 0 + kYccBias[c]) >> 16; } // RGB (0, 255, 0)

// what the kernels need of a packed colour family (ck_raw_class: bpp 2 with the luma's byte offset in k[2], bpp 3 / 4 with the luma
// weight of a pixel's bytes 0, 1, 2: the weight of byte 0 tells RGB from BGR)
// identity: the weights that hand a packed colour family's own R, G, B bytes through instead (the coloured-piece detector, §4r)
void color_source(const ck_raw_geom &L, int orientation, const uint8_t *p, int stride, size_t pitch, bool identity, ck_pv_csrc *cs) {
    memset(cs, 0, sizeof *cs);
    cs->p = p; cs->stride = stride; cs->pitch = pitch;
    cs->sw = L.sw; cs->sh = L.sh; cs->orientation = orientation; cs->bpp = L.cls.bpp;
    if (L.cls.bpp == 2) { // YUYV: Y0 U Y1 V, UYVY: U Y0 V Y1
        const int yo = (int)L.cls.k[2];
        cs->off[0] = yo; cs->off[1] = 1 - yo; cs->off[2] = 3 - yo;
    }
    const bool bgr = L.cls.k[0] == CK_LUMA_B;
    for (int c = 0; c < 3; c++) {
        for (int k = 0; k < 3; k++) cs->wgt[c][k] = identity ? ((bgr ? 2 - k : k) == c ? 65536 : 0) : kYcc[c][bgr ? 2 - k : k];
        cs->bias[c] = identity ? 0 : kYccBias[c];
        cs->ovl[c] = overlay_component(c);
    }
}

// the plane map of a planar 4:2:0 frame (ck_raw_planes.h) as the kernels take it
void planar_source(const ckp_map &m, int turn, const uint8_t *p, size_t pitch, ck_pv_psrc *ps) {
    memset(ps, 0, sizeof *ps);
    ps->p = p; ps->pitch = pitch;
    ps->sw = m.sw; ps->sh = m.sh; ps->orientation = turn;
    for (int c = 0; c < 3; c++) {
        ps->off[c] = (int)m.c[c].off; ps->rstride[c] = m.c[c].row_stride; ps->step[c] = m.c[c].step;
        ps->cs[c] = m.c[c].cs; ps->rs[c] = m.c[c].rs;
        ps->ovl[c] = overlay_component(c);
    }
}

} // namespace

// The source of a colour call as the kernels take it, checked in the contract's order; *n_avail: the frames an index may name.
int ck_pv_source(ck_handle *h, const ck_pv_color_src &src, bool identity, ck_pv_any *store, ck_pv_src *any, int *n_avail) {
    *any = {nullptr, nullptr, nullptr};
    if (src.jpeg) { // the frames of a JPEG decode in the colour form (§4i)
        const ck_jpeg_color_src &J = *src.jpeg;
        store->js = {J.img.p, J.img.stride, J.img.pitch, J.descs, J.status, J.planes, J.sw, J.sh, J.orientation, {overlay_component(0), overlay_component(1), overlay_component(2)}};
        any->jpeg = &store->js;
        *n_avail = J.n_frames;
        return CK_OK;
    }
    ck_raw_geom L;
    const int rc = ck_raw_geometry(src.fmt, h->w, h->h, &L);
    if (rc != CK_OK) return rc;
    if (L.cls.bpp == 1 && !L.planes) return CK_EUNSUPPORTED; // a luma-first family without CK_RAW_PLANES: its chroma is not part of the frame (the grey preview serves it)
    if ((!src.p && src.n_frames > 0) || src.n_frames < 0 || !ck_raw_pitch_ok(L, src.stride, src.pitch)) return CK_EINVAL;
    *n_avail = src.n_frames;
    if (L.planes) {
        ckp_map m;
        if (ckp_map_make(L.planes, L.sw, L.sh, src.stride, &m) != 0) return CK_EINVAL;
        if (m.bytes > INT32_MAX) return CK_ECAPACITY; // the kernels place a sample of a frame in 32 bits
        planar_source(m, L.turn, src.p, (size_t)src.pitch, &store->ps);
        any->planar = &store->ps;
        return CK_OK;
    }
    color_source(L, L.turn, src.p, src.stride, (size_t)src.pitch, identity, &store->cs);
    any->raw = &store->cs;
    return CK_OK;
}

// The one-thread host twin of the colour triples (§4g, §4s): what k_pv_color writes at the identity size without overlay.
extern "C" int ck_raw_ycc_host(const ck_raw_format_t *fmt, const ck_image_u8_t *imgs, int32_t n, int32_t W, int32_t H, uint8_t *ycc_out) {
    ck_raw_geom L;
    const int rc = ck_raw_geometry(fmt, W, H, &L);
    if (rc != CK_OK) return rc;
    if (L.cls.bpp == 1 && !L.planes) return CK_EUNSUPPORTED;
    if (n < 0 || (n > 0 && !imgs) || !ycc_out) return CK_EINVAL;
    for (int i = 0; i < n; i++)
        if (!imgs[i].buf || imgs[i].width != L.sw || imgs[i].height != L.sh || !ck_raw_stride_ok(L, imgs[i].stride)) return CK_EINVAL;
    for (int i = 0; i < n; i++) {
        const uint8_t *S = imgs[i].buf;
        uint8_t *out = ycc_out + (size_t)i * W * H * 3;
        ckp_map m;
        ck_pv_csrc cs;
        if (L.planes) { if (ckp_map_make(L.planes, L.sw, L.sh, imgs[i].stride, &m) != 0) return CK_EINVAL; }
        else color_source(L, L.turn, S, imgs[i].stride, 0, false, &cs);
        for (int oy = 0; oy < H; oy++)
            for (int ox = 0; ox < W; ox++, out += 3) {
                int32_t u, v;
                ckp_source_xy(L.turn, L.sw, L.sh, ox, oy, &u, &v);
                if (L.planes) { ckp_triple(&m, S, u, v, out); continue; }
                const uint8_t *row = S + (size_t)v * imgs[i].stride;
                for (int c = 0; c < 3; c++) {
                    if (cs.bpp == 2) { out[c] = row[(c ? (u >> 1) << 2 : u << 1) + cs.off[c]]; continue; }
                    const uint8_t *px = row + (size_t)u * cs.bpp;
                    out[c] = (uint8_t)((cs.wgt[c][0] * px[0] + cs.wgt[c][1] * px[1] + cs.wgt[c][2] * px[2] + cs.bias[c]) >> 16);
                }
            }
    }
    return CK_OK;
}

int ck_preview_color_run(ck_handle *h, const ck_preview_params_t *pp, const ck_pv_color_src &src, const int32_t *frames, int32_t n,
                         uint8_t *out, bool files, int64_t cap_per_frame, int64_t *sizes, uint32_t *status) {
    if (!h || !pp || !out || n < 0 || (files && (!sizes || cap_per_frame < 1))) return CK_EINVAL;
    ck_pv_geom g;
    int rc = resolve(pp, h->w, h->h, 3, &g);
    if (rc != CK_OK) return rc;
    ck_pv_any store;
    ck_pv_src any;
    int n_avail;
    rc = ck_pv_source(h, src, false, &store, &any, &n_avail);
    if (rc == CK_OK) rc = begin(h, frames, n, n_avail, &g);
    if (rc != CK_OK || n == 0) return rc;
    if (files) return encode_files(h, pp, g, &any, n, out, cap_per_frame, sizes, status);
    return read_pixels(h, (size_t)g.pw * g.ph * 3 * n, out, [&](uint8_t *d) { return ck_launch_preview_color(h, g, any, n, d); });
}

static_assert(sizeof(ck_preview_params_t) == 24, "ck_preview_params_t layout");

extern "C" void ck_preview_params_default(ck_preview_params_t *pp) {
    if (!pp) return;
    memset(pp, 0, sizeof *pp);
    pp->width = 640; pp->height = 480; // the caps filter of the reference's stream (mjpeg.rs:41-49)
    pp->quality = 50;                  // turbojpeg::compress(.., 50, ..) (mjpeg.rs:116)
}

static int layout(const ck_preview_params_t *pp, int32_t W, int32_t H, int nc, int32_t *pw, int32_t *ph, int64_t *max_bytes) {
    ck_pv_geom g;
    const int rc = resolve(pp, W, H, nc, &g);
    if (rc != CK_OK) return rc;
    if (pw) *pw = g.pw;
    if (ph) *ph = g.ph;
    if (max_bytes) *max_bytes = max_file_bytes(g);
    return CK_OK;
}
extern "C" int ck_preview_layout(const ck_preview_params_t *pp, int32_t W, int32_t H, int32_t *pw, int32_t *ph, int64_t *max_bytes) {
    return layout(pp, W, H, 1, pw, ph, max_bytes);
}
extern "C" int ck_preview_color_layout(const ck_preview_params_t *pp, int32_t W, int32_t H, int32_t *pw, int32_t *ph, int64_t *max_bytes) {
    return layout(pp, W, H, 3, pw, ph, max_bytes);
}

extern "C" int ck_preview_luma(ck_handle_t *h, const ck_preview_params_t *pp, const int32_t *frames, int32_t n, uint8_t *out) {
    ck_pv_geom g;
    const int rc = begin(h, pp, frames, n, out, &g);
    if (rc != CK_OK || n == 0) return rc;
    return read_pixels(h, (size_t)g.pw * g.ph * n, out, [&](uint8_t *d) { return ck_launch_preview_luma(h, g, n, d); });
}

extern "C" int ck_preview_jpeg(ck_handle_t *h, const ck_preview_params_t *pp, const int32_t *frames, int32_t n, uint8_t *out,
                               int64_t cap_per_frame, int64_t *sizes, uint32_t *status) {
    if (!sizes || cap_per_frame < 1) return CK_EINVAL;
    ck_pv_geom g;
    const int rc = begin(h, pp, frames, n, out, &g);
    if (rc != CK_OK || n == 0) return rc;
    return encode_files(h, pp, g, nullptr, n, out, cap_per_frame, sizes, status);
}

// ---- colour (§4g): the raw frames of the handle's staging, or of the caller's device memory ---------------------------------------
// the colour source behind the staged frames: their raw twin, while the last ck_upload_raw / ck_raw_luma_batch still is what staged
// them; or the chroma planes beside them, while the last ck_upload_jpeg_color is (*js is then what src->jpeg points to)
int ck_pv_staged_source(ck_handle *h, ck_pv_color_src *src, ck_jpeg_color_src *js) {
    if (!h) return CK_EINVAL;
    if (h->n_jpeg_color >= 0) {
        const int rc = ck_jpeg_color_source(h, js);
        *src = {nullptr, 0, 0, js->n_frames, nullptr, js};
        return rc;
    }
    if (h->n_raw_staged < 0) return CK_EINVAL;
    ck_raw_geom L;
    const int rc = ck_raw_geometry(&h->raw_staged_fmt, h->w, h->h, &L);
    if (rc != CK_OK) return rc;
    *src = {h->n_raw_staged ? (const uint8_t *)h->raw->d_stage : nullptr, L.stride16, (int64_t)L.pitch16, h->n_raw_staged, &h->raw_staged_fmt, nullptr};
    return CK_OK;
}

extern "C" int ck_preview_jpeg_color(ck_handle_t *h, const ck_preview_params_t *pp, const int32_t *frames, int32_t n, uint8_t *out,
                                     int64_t cap_per_frame, int64_t *sizes, uint32_t *status) {
    ck_pv_color_src src;
    ck_jpeg_color_src js;
    const int rc = ck_pv_staged_source(h, &src, &js);
    return rc != CK_OK ? rc : ck_preview_color_run(h, pp, src, frames, n, out, true, cap_per_frame, sizes, status);
}
extern "C" int ck_preview_color(ck_handle_t *h, const ck_preview_params_t *pp, const int32_t *frames, int32_t n, uint8_t *out) {
    ck_pv_color_src src;
    ck_jpeg_color_src js;
    const int rc = ck_pv_staged_source(h, &src, &js);
    return rc != CK_OK ? rc : ck_preview_color_run(h, pp, src, frames, n, out, false, 0, nullptr, nullptr);
}
extern "C" int ck_preview_jpeg_color_device(ck_handle_t *h, const ck_preview_params_t *pp, const uint8_t *d_raw, int32_t stride,
                                            int64_t frame_pitch, const ck_raw_format_t *fmt, const int32_t *frames, int32_t n_frames,
                                            int32_t n, uint8_t *out, int64_t cap_per_frame, int64_t *sizes, uint32_t *status) {
    return ck_preview_color_run(h, pp, {d_raw, stride, frame_pitch, n_frames, fmt, nullptr}, frames, n, out, true, cap_per_frame, sizes, status);
}
extern "C" int ck_preview_color_device(ck_handle_t *h, const ck_preview_params_t *pp, const uint8_t *d_raw, int32_t stride,
                                       int64_t frame_pitch, const ck_raw_format_t *fmt, const int32_t *frames, int32_t n_frames, int32_t n,
                                       uint8_t *out) {
    return ck_preview_color_run(h, pp, {d_raw, stride, frame_pitch, n_frames, fmt, nullptr}, frames, n, out, false, 0, nullptr, nullptr);
}
