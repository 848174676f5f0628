// Exposure metering of the staged frames: what ck_exposure.hip (host) and k_exposure.hip (kernel) share.
#ifndef CK_EXPOSURE_H
#define CK_EXPOSURE_H

#include "ck_grow.h"

#define CK_EX_TW 128 /* pixels of a tile, one 256-thread workgroup each: 32 column groups of 4 pixels x 8 row groups */
#define CK_EX_TH 64

// one entry of a call: the frame it meters and its rectangle, clamped to the frame on the host (x0 >= x1 or y0 >= y1: empty)
struct ck_ex_job { int32_t frame, x0, y0, x1, y1; };

// Workspace, allocated by the first exposure call and grown on demand (ck_create allocates none of it)
struct ck_exposure_ws {
    ck_dev_buf<ck_exposure_stats_t> d_stats;    // [n] the records the kernel accumulates into
    ck_dev_buf<uint8_t> d_tab;                  // the gamma tables [CK_EXPOSURE_GAMMAS][256], then [n] ck_ex_job
    ck_pinned_buf<uint8_t> h_tab;               // pinned mirror of d_tab
    ck_pinned_buf<ck_exposure_stats_t> h_stats; // pinned landing of the records
};

// k_exposure.hip: zeroes the n records and accumulates them, on `stream`
int ck_launch_exposure(hipStream_t stream, const ck_dev_image &img, int w, int h, int n, const uint8_t *d_lut, const ck_ex_job *d_jobs,
                       ck_exposure_stats_t *d_stats);
// ck_exposure.hip: the one path of ck_exposure_stats / ck_exposure_stats_ingested; n_avail = frames `img` holds
int ck_exposure_run(ck_handle *h, const ck_dev_image &img, int n_avail, const int32_t *frames, int32_t n, const ck_exposure_params_t *p,
                    const ck_rect_t *roi, ck_exposure_stats_t *out);

#endif
