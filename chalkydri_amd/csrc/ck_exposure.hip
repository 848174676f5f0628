// Exposure metering of the staged frames: the host half that drives the device.  Validates a call, clamps the
// rectangles, hands the gamma tables (ck_exposure_luts) and the job list to the kernel of k_exposure.hip on the handle's stream and
// brings the records back; the arithmetic on the records is ck_exposure_host.c's.
#include <string.h>

#include "ck_exposure.h"

static constexpr size_t kLutBytes = (size_t)CK_EXPOSURE_GAMMAS * 256;

int ck_exposure_run(ck_handle *h, const ck_dev_image &img, int n_avail, const int32_t *frames, int32_t n, const ck_exposure_params_t *p,
                    const ck_rect_t *roi, ck_exposure_stats_t *out) {
    if (!h || !p || !out || n < 0) return CK_EINVAL;
    uint8_t lut[kLutBytes];
    int rc = ck_exposure_luts(p, lut); // (the parameter checks are the host functions': one place)
    if (rc != CK_OK) return rc;
    if (n > h->cfg.max_batch) return CK_ECAPACITY;
    if (!ck_frame_list_ok(frames, n, n_avail)) return CK_EINVAL;
    if (n == 0) return CK_OK;
    CK_HIP(hipSetDevice(h->device));
    if (!ck_workspace(h->exposure)) return CK_ENOMEM;
    ck_exposure_ws &E = *h->exposure;
    const size_t tab_bytes = kLutBytes + sizeof(ck_ex_job) * (size_t)n, stats_bytes = sizeof(ck_exposure_stats_t) * (size_t)n;
    rc = E.d_stats.reserve(stats_bytes);
    if (rc == CK_OK) rc = E.d_tab.reserve(tab_bytes);
    if (rc == CK_OK) rc = E.h_tab.reserve(tab_bytes);
    if (rc == CK_OK) rc = E.h_stats.reserve(stats_bytes);
    if (rc != CK_OK) return rc;
    memcpy(E.h_tab, lut, kLutBytes); // (pinned; every call ends with a synchronisation, so the last call's copy is done)
    ck_ex_job *jobs = reinterpret_cast<ck_ex_job *>(E.h_tab + kLutBytes);
    for (int i = 0; i < n; i++) {
        ck_ex_job &j = jobs[i];
        j.frame = frames ? frames[i] : i;
        j.x0 = 0; j.y0 = 0; j.x1 = h->w; j.y1 = h->h;
        if (roi) { // clamped to the frame; a rectangle that is empty then stays empty for the kernel (x0 >= x1 or y0 >= y1)
            j.x0 = roi[i].x0 < 0 ? 0 : (roi[i].x0 > h->w ? h->w : roi[i].x0);
            j.y0 = roi[i].y0 < 0 ? 0 : (roi[i].y0 > h->h ? h->h : roi[i].y0);
            j.x1 = roi[i].x1 < 0 ? 0 : (roi[i].x1 > h->w ? h->w : roi[i].x1);
            j.y1 = roi[i].y1 < 0 ? 0 : (roi[i].y1 > h->h ? h->h : roi[i].y1);
        }
    }
    CK_HIP(hipMemcpyAsync(E.d_tab, E.h_tab, tab_bytes, hipMemcpyHostToDevice, h->stream));
    rc = ck_launch_exposure(h->stream, img, h->w, h->h, n, E.d_tab, reinterpret_cast<const ck_ex_job *>(E.d_tab + kLutBytes), E.d_stats);
    if (rc != CK_OK) return rc;
    CK_HIP(hipMemcpyAsync(E.h_stats, E.d_stats, stats_bytes, hipMemcpyDeviceToHost, h->stream));
    CK_HIP(hipStreamSynchronize(h->stream));
    memcpy(out, E.h_stats, stats_bytes);
    return CK_OK;
}

extern "C" int ck_exposure_stats(ck_handle_t *h, const int32_t *frames, int32_t n, const ck_exposure_params_t *p, const ck_rect_t *roi,
                                 ck_exposure_stats_t *out) {
    if (!h) return CK_EINVAL;
    return ck_exposure_run(h, ck_staged_image(h), h->n_staged, frames, n, p, roi, out);
}
