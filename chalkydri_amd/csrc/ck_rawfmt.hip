// ck_rawfmt.hip — raw camera formats and orientation: the host half.  Validates format and geometry, packs host
// frames into one pinned staging buffer (rows at the minimum stride rounded up to 16, so the device side is aligned whatever the
// caller's stride and base were), copies it with one asynchronous copy and runs k_rawfmt.hip into the staged frames.
#include <string.h>

#include "ck_internal.h"
#include "ck_rawfmt.h"
#include "ck_raw_planes.h"

namespace {

constexpr uint32_t cc4(const char (&s)[5]) {
    return (uint32_t)(uint8_t)s[0] | ((uint32_t)(uint8_t)s[1] << 8) | ((uint32_t)(uint8_t)s[2] << 16) | ((uint32_t)(uint8_t)s[3] << 24);
}

int check_raw_imgs(const ck_handle *h, const ck_image_u8_t *imgs, int n, const ck_raw_format_t *fmt, ck_raw_geom *L) {
    if (!h) return CK_EINVAL;
    const int rc = ck_raw_geometry(fmt, h->w, h->h, L);
    if (rc != CK_OK) return rc;
    if (n < 0 || (n > 0 && !imgs)) return CK_EINVAL;
    if (n > h->cfg.max_batch) return CK_ECAPACITY;
    for (int i = 0; i < n; i++)
        if (!imgs[i].buf || imgs[i].width != L->sw || imgs[i].height != L->sh || !ck_raw_stride_ok(*L, imgs[i].stride)) return CK_EINVAL;
    return CK_OK;
}

// host frames -> staging -> device -> staged frames, enqueued on the handle's stream (the caller synchronises)
int stage_and_convert(ck_handle *h, const ck_image_u8_t *imgs, int n, const ck_raw_format_t *fmt, const ck_raw_geom &L) {
    CK_HIP(hipSetDevice(h->device));
    h->n_raw_staged = -1; // the raw staging is about to be rewritten: its twin is valid again only once this call has succeeded
    if (n == 0) { ck_set_staged(h, 0); h->n_raw_staged = 0; h->raw_staged_fmt = *fmt; return CK_OK; }
    // exactly these bytes: under CK_POISON=3 the device buffer then ends where the kernel's last permitted read ends
    // (with chroma planes the last frame ends with the last sample of its last plane: ckp_extent)
    const size_t st = (size_t)L.stride16, pitch = L.pitch16;
    size_t last = pitch - st + L.min_stride;
    if (L.planes) {
        ckp_map m;
        if (ckp_map_make(L.planes, L.sw, L.sh, L.stride16, &m) != 0) return CK_EINVAL;
        last = (size_t)ckp_extent(&m);
    }
    const size_t bytes = pitch * (n - 1) + last;
    if (!ck_workspace(h->raw)) return CK_ENOMEM;
    ck_raw_ws &R = *h->raw;
    int rc = R.h_stage.reserve(bytes, true);
    if (rc == CK_OK) rc = R.d_stage.reserve(bytes, true);
    if (rc != CK_OK) return rc;
    for (int i = 0; i < n; i++) {
        uint8_t *dst = R.h_stage + (size_t)i * pitch;
        if (L.planes) ckp_copy(L.planes, L.sw, L.sh, imgs[i].buf, imgs[i].stride, dst, L.stride16);
        else if ((size_t)imgs[i].stride == st) memcpy(dst, imgs[i].buf, last);
        else for (int y = 0; y < L.sh; y++) memcpy(dst + (size_t)y * st, imgs[i].buf + (size_t)y * imgs[i].stride, (size_t)L.min_stride);
    }
    CK_HIP(hipMemcpyAsync(R.d_stage, R.h_stage, bytes, hipMemcpyHostToDevice, h->stream));
    rc = ck_launch_rawfmt(h, h->stream, {R.d_stage, (int)st, pitch, L.sw, L.sh}, L.cls, L.turn, h->d_frames, n);
    if (rc != CK_OK) return rc;
    ck_set_staged(h, n);
    h->n_raw_staged = n; // (d_stage keeps the raw frames: the colour preview's source)
    h->raw_staged_fmt = *fmt;
    return CK_OK;
}

} // namespace

int ck_raw_classify(uint32_t fourcc, ck_raw_class *out) {
    const uint32_t R = CK_LUMA_R, G = CK_LUMA_G, B = CK_LUMA_B;
    switch (fourcc) {
    case cc4("GREY"): case cc4("GRAY"): case cc4("Y800"): *out = {1, {CKP_NONE, 0, 0}}; return CK_OK;
    case cc4("NV12"): *out = {1, {CKP_NV12, 0, 0}}; return CK_OK;
    case cc4("NV21"): *out = {1, {CKP_NV21, 0, 0}}; return CK_OK;
    case cc4("I420"): *out = {1, {CKP_I420, 0, 0}}; return CK_OK;
    case cc4("YV12"): *out = {1, {CKP_YV12, 0, 0}}; return CK_OK;
    // v_perm_b32 selectors: bytes 0..3 = the first dword of a pair, 4..7 = the second
    case cc4("YUYV"): case cc4("YUY2"): *out = {2, {0x06040200u, 0x00020406u, 0}}; return CK_OK;
    case cc4("UYVY"): *out = {2, {0x07050301u, 0x01030507u, 1}}; return CK_OK;
    case cc4("RGB3"): case cc4("RGB "): *out = {3, {R, G, B}}; return CK_OK;
    case cc4("BGR3"): case cc4("BGR "): *out = {3, {B, G, R}}; return CK_OK;
    case cc4("RGBA"): *out = {4, {R, G, B}}; return CK_OK;
    case cc4("BGRA"): *out = {4, {B, G, R}}; return CK_OK;
    }
    return CK_EUNSUPPORTED;
}

int ck_raw_geometry(const ck_raw_format_t *fmt, int w, int h, ck_raw_geom *L) {
    if (!fmt || w < 1 || h < 1) return CK_EINVAL;
    const int rc = ck_raw_classify(fmt->fourcc, &L->cls);
    if (rc != CK_OK) return rc;
    if (fmt->orientation & ~(3 | CK_RAW_PLANES)) return CK_EINVAL; // (a negative value has high bits set)
    L->turn = fmt->orientation & 3;
    const bool flag = (fmt->orientation & CK_RAW_PLANES) != 0;
    L->planes = flag && L->cls.bpp == 1 ? (int)L->cls.k[0] : CKP_NONE;
    if (flag && !L->planes) return CK_EUNSUPPORTED; // GREY and the packed families have no planes behind them
    if (L->cls.bpp == 1) L->cls.k[0] = (uint32_t)L->planes;
    ck_source_size(w, h, L->turn, &L->sw, &L->sh);
    L->ch = L->planes ? (L->sh + 1) / 2 : 0;
    L->min_stride = L->planes ? ckp_min_stride(L->sw) : (L->cls.bpp == 2 ? 4 * ((L->sw + 1) / 2) : L->cls.bpp * L->sw);
    L->stride16 = (L->min_stride + 15) / 16 * 16;
    L->pitch16 = (size_t)L->stride16 * (L->sh + L->ch);
    return CK_OK;
}

extern "C" int ck_raw_layout(const ck_raw_format_t *fmt, int32_t width, int32_t height, int32_t *sw, int32_t *sh, int32_t *min_stride,
                             int64_t *min_bytes) {
    if (!sw || !sh || !min_stride || !min_bytes) return CK_EINVAL;
    ck_raw_geom L;
    const int rc = ck_raw_geometry(fmt, width, height, &L);
    if (rc != CK_OK) return rc;
    *sw = L.sw; *sh = L.sh; *min_stride = L.min_stride;
    *min_bytes = (int64_t)(L.sh + L.ch) * L.min_stride;
    return CK_OK;
}

extern "C" int ck_upload_raw(ck_handle_t *h, const ck_image_u8_t *imgs, int32_t n, const ck_raw_format_t *fmt) {
    ck_raw_geom L;
    int rc = check_raw_imgs(h, imgs, n, fmt, &L);
    if (rc != CK_OK) return rc;
    rc = stage_and_convert(h, imgs, n, fmt, L);
    if (rc != CK_OK) return rc;
    CK_HIP(hipStreamSynchronize(h->stream)); // (the staging buffer is free again, and ck_upload_frames returns staged frames too)
    return CK_OK;
}

extern "C" int ck_raw_luma_batch(ck_handle_t *h, const ck_image_u8_t *imgs, int32_t n, const ck_raw_format_t *fmt, uint8_t *luma_out) {
    if (!luma_out) return CK_EINVAL;
    ck_raw_geom L;
    int rc = check_raw_imgs(h, imgs, n, fmt, &L);
    if (rc != CK_OK) return rc;
    rc = stage_and_convert(h, imgs, n, fmt, L);
    if (rc != CK_OK) return rc;
    rc = ck_read_staged_luma(h, n, luma_out);
    if (rc != CK_OK) return rc;
    CK_HIP(hipStreamSynchronize(h->stream));
    return CK_OK;
}

extern "C" int ck_upload_raw_device(ck_handle_t *h, const uint8_t *d_raw, int32_t n, int32_t stride, int64_t frame_pitch,
                                    const ck_raw_format_t *fmt) {
    if (!h) return CK_EINVAL;
    ck_raw_geom L;
    int rc = ck_raw_geometry(fmt, h->w, h->h, &L);
    if (rc != CK_OK) return rc;
    if (!d_raw || n < 0 || !ck_raw_pitch_ok(L, stride, frame_pitch)) return CK_EINVAL;
    if (n > h->cfg.max_batch) return CK_ECAPACITY;
    CK_HIP(hipSetDevice(h->device));
    rc = ck_launch_rawfmt(h, h->stream, {d_raw, stride, (size_t)frame_pitch, L.sw, L.sh}, L.cls, L.turn, h->d_frames, n);
    if (rc != CK_OK) return rc;
    CK_HIP(hipStreamSynchronize(h->stream)); // (the caller may reuse d_raw)
    ck_set_staged(h, n);
    return CK_OK;
}

static_assert(sizeof(ck_raw_planes_t) == 80, "ck_raw_planes_t layout");

extern "C" int ck_raw_plane_layout(const ck_raw_format_t *fmt, int32_t width, int32_t height, int32_t stride, ck_raw_planes_t *out) {
    if (!out) return CK_EINVAL;
    ck_raw_geom L;
    const int rc = ck_raw_geometry(fmt, width, height, &L);
    if (rc != CK_OK) return rc;
    if (!L.planes) return CK_EUNSUPPORTED;
    ckp_map m;
    if (ckp_map_make(L.planes, L.sw, L.sh, stride, &m) != 0) return CK_EINVAL;
    memset(out, 0, sizeof *out);
    out->sw = m.sw; out->sh = m.sh; out->cw = m.cw; out->ch = m.ch;
    for (int c = 0; c < 3; c++) { out->offset[c] = m.c[c].off; out->row_stride[c] = m.c[c].row_stride; out->step[c] = m.c[c].step; }
    out->bytes = m.bytes;
    return CK_OK;
}
