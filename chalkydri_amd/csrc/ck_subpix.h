// Sub-pixel corners: what ck_subpix.hip, ck_subpix_host.c and the pipeline (ck_stages.hip) share.
#ifndef CK_SUBPIX_H
#define CK_SUBPIX_H

#include "chalkydri_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
// ck_subpix_host.c: the checks every entry point shares
int ck_subpix_params_check(const ck_subpix_params_t *pp);
int ck_subpix_point_ok(double x, double y, int width, int height);
int ck_board_check(const ck_board_t *b, const ck_board_params_t *bp, int n_families); // n_families < 0: no handle to hold the family against
#ifdef __cplusplus
}

#include "ck_grow.h"

// allocated by the first call that needs it (ck_corner_subpix, ck_set_corner_subpix, ck_board_corners_last), grown on demand
struct ck_subpix_ws {
    // the detector setting: its parameters live in the handle, its weight table here
    ck_dev_buf<double> d_set_wts;
    // ck_corner_subpix / ck_board_corners_last: the call's weight table and whatever of its arrays is not on the device already
    ck_dev_buf<double> d_wts, d_in, d_out;
    ck_dev_buf<int32_t> d_frame, d_ntags;
    ck_dev_buf<ck_subpix_info_t> d_info;
    ck_dev_buf<uint8_t> d_state;
};

// k_subpix_dets over the detections run_tail just left in ws.d_dets for frames [0, n) of img, on h->stream (the setting is on)
int ck_launch_subpix_dets(ck_handle *h, const ck_dev_image &img, int n);
#endif

#endif
