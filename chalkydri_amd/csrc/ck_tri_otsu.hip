// Iterative tri-class Otsu threshold: the host half that drives the device.  Validates a call, grows the workspace,
// stages what lies in host memory (arrays on the handle's device are used in place), runs the three kernels of k_tri_otsu.hip on
// the handle's stream and brings the results to where the caller wants them.
#include "ck_tri_otsu.h"

static_assert(sizeof(ck_tri_otsu_params_t) == 16, "ck_tri_otsu_params_t layout");
static_assert(sizeof(ck_tri_otsu_info_t) == 160, "ck_tri_otsu_info_t layout");

// memory of the handle's device that a kernel may use as it is; anything else goes through a copy
static bool on_device(const void *p, int device) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError(); // (pageable host memory is unknown to the runtime: an error here, not a failure of the call)
        return false;
    }
    return a.type == hipMemoryTypeDevice && a.device == device;
}

extern "C" int ck_cat_tri_otsu_batch(ck_handle_t *h, const ck_tri_otsu_params_t *p, const uint8_t *px, int32_t n, int32_t w, int32_t ht,
                                     uint8_t *classes_out, ck_tri_otsu_info_t *info_out, uint32_t *hist_out) {
    if (!h || !px || !classes_out || n < 0 || w < 1 || ht < 1) return CK_EINVAL;
    if (!ck_tri_otsu_params_ok(p)) return CK_EINVAL;
    const size_t npix = (size_t)w * (size_t)ht;
    if (npix >= ((size_t)1 << 31)) return CK_EINVAL; // a frame's counts are 32 bits
    if (n == 0) return CK_OK;
    CK_HIP(hipSetDevice(h->device));
    if (!ck_workspace(h->tri_otsu)) return CK_ENOMEM;
    ck_tri_otsu_ws &W = *h->tri_otsu;
    const size_t cls_bytes = npix * (size_t)n, px_bytes = cls_bytes * (size_t)p->channels;
    const bool px_here = on_device(px, h->device), cls_here = on_device(classes_out, h->device);
    int rc = W.d_hist.reserve(sizeof(uint32_t) * 256 * (size_t)n);
    if (rc == CK_OK) rc = W.d_lut.reserve((size_t)256 * (size_t)n);
    if (rc == CK_OK) rc = W.d_info.reserve(sizeof(ck_tri_otsu_info_t) * (size_t)n);
    if (rc == CK_OK && !px_here) rc = W.d_px.reserve(px_bytes);
    if (rc == CK_OK && !cls_here) rc = W.d_cls.reserve(cls_bytes);
    if (rc != CK_OK) return rc;
    const uint8_t *d_px = px;
    if (!px_here) {
        CK_HIP(hipMemcpyAsync(W.d_px, px, px_bytes, hipMemcpyDefault, h->stream));
        d_px = W.d_px;
    }
    uint8_t *d_cls = cls_here ? classes_out : W.d_cls.p;
    rc = ck_launch_tri_otsu(h->stream, *p, d_px, n, npix, d_cls, W.d_hist, W.d_lut, W.d_info);
    if (rc != CK_OK) return rc;
    if (!cls_here) CK_HIP(hipMemcpyAsync(classes_out, d_cls, cls_bytes, hipMemcpyDefault, h->stream));
    if (info_out) CK_HIP(hipMemcpyAsync(info_out, W.d_info, sizeof(ck_tri_otsu_info_t) * (size_t)n, hipMemcpyDefault, h->stream));
    if (hist_out) CK_HIP(hipMemcpyAsync(hist_out, W.d_hist, sizeof(uint32_t) * 256 * (size_t)n, hipMemcpyDefault, h->stream));
    CK_HIP(hipStreamSynchronize(h->stream));
    return CK_OK;
}

extern "C" int ck_cat_tri_otsu(ck_handle_t *h, const uint8_t *rgb, int32_t w, int32_t ht, uint8_t *classes_out) {
    ck_tri_otsu_params_t p;
    ck_tri_otsu_params_default(&p);
    return ck_cat_tri_otsu_batch(h, &p, rgb, 1, w, ht, classes_out, nullptr, nullptr);
}
