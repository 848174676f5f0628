// Exposure metering of the staged frames: the host half that drives the device.  Validates a call, clamps the
// rectangles, hands the gamma tables (ck_exposure_luts) and the job list to the kernel of k_exposure.hip on the handle's stream and
// brings the records back; the arithmetic on the records is ck_exposure_host.c's.
#include <new>
#include <string.h>

#include "ck_exposure.h"

namespace {

constexpr size_t kLutBytes = (size_t)CK_EXPOSURE_GAMMAS * 256;

int grow_dev(void **p, size_t *cap, size_t need) { // capacities in bytes
    if (need <= *cap) return CK_OK;
    (void)ck_free_dev(*p);
    *p = nullptr; *cap = 0;
    const size_t want = need + need / 4;
    uint8_t *q = nullptr;
    CK_HIP_ALLOC(ck_malloc_dev(&q, want));
    *p = q; *cap = want;
    return CK_OK;
}

int grow_host(void **p, size_t *cap, size_t need) {
    if (need <= *cap) return CK_OK;
    if (*p) (void)hipHostFree(*p);
    *p = nullptr; *cap = 0;
    const size_t want = need + need / 4;
    if (hipHostMalloc(p, want, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
        return CK_ENOMEM;
    }
    *cap = want;
    return CK_OK;
}

} // namespace

void ck_exposure_free(ck_handle *h) {
    if (!h || !h->exposure) return;
    ck_exposure_ws &E = *h->exposure;
    if (E.h_tab) (void)hipHostFree(E.h_tab);
    if (E.h_stats) (void)hipHostFree(E.h_stats);
    (void)ck_free_dev(E.d_stats); (void)ck_free_dev(E.d_tab);
    delete h->exposure;
    h->exposure = nullptr;
}

int ck_exposure_run(ck_handle *h, const ck_dev_image &img, int n_avail, const int32_t *frames, int32_t n, const ck_exposure_params_t *p,
                    const ck_rect_t *roi, ck_exposure_stats_t *out) {
    if (!h || !p || !out || n < 0) return CK_EINVAL;
    uint8_t lut[kLutBytes];
    int rc = ck_exposure_luts(p, lut); // (the parameter checks are the host functions': one place)
    if (rc != CK_OK) return rc;
    if (n > h->cfg.max_batch) return CK_ECAPACITY;
    for (int i = 0; i < n; i++) {
        const int f = frames ? frames[i] : i;
        if (f < 0 || f >= n_avail) return CK_EINVAL;
    }
    if (n == 0) return CK_OK;
    CK_HIP(hipSetDevice(h->device));
    if (!h->exposure) {
        h->exposure = new (std::nothrow) ck_exposure_ws();
        if (!h->exposure) return CK_ENOMEM;
        memset(h->exposure, 0, sizeof *h->exposure);
    }
    ck_exposure_ws &E = *h->exposure;
    const size_t tab_bytes = kLutBytes + sizeof(ck_ex_job) * (size_t)n, stats_bytes = sizeof(ck_exposure_stats_t) * (size_t)n;
    rc = grow_dev(reinterpret_cast<void **>(&E.d_stats), &E.stats_cap, stats_bytes);
    if (rc == CK_OK) rc = grow_dev(reinterpret_cast<void **>(&E.d_tab), &E.tab_cap, tab_bytes);
    if (rc == CK_OK) rc = grow_host(reinterpret_cast<void **>(&E.h_tab), &E.h_tab_cap, tab_bytes);
    if (rc == CK_OK) rc = grow_host(reinterpret_cast<void **>(&E.h_stats), &E.h_stats_cap, stats_bytes);
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
