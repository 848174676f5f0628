// Mount calibration: what ck_rigcal.hip (host) and k_rigcal.hip (kernel) share; ck_rigcal_c.h is the part the host
// twin (plain C) shares too.
#ifndef CK_RIGCAL_H
#define CK_RIGCAL_H

#include "ck_grow.h"
#include "ck_rigcal_c.h"

// One problem as the kernel sees it
struct ck_rigcal_dev_problem {
    int64_t index_off; // int32 entries into d_index (cka_index_at over n_used, n_views)
    int32_t step_off;  // records into d_steps
    int32_t view_off;  // records into d_views
    int32_t n_used, n_views;
    uint64_t mask;     // ck_rigcal_plan_t::mask
};

// Workspace, allocated by the first mount calibration call and grown on demand (ck_create allocates none of it)
struct ck_rigcal_ws {
    ck_dev_buf<ck_rigcal_dev_problem> d_prob; // [n_problems]
    ck_dev_buf<int32_t> d_tab;                // [n_cams * n_steps][3] the capture's view table (ck_rigcal_table)
    ck_dev_buf<int32_t> d_index;              // the problems' arrowhead indices (ck_cal_math.h), one after the other
    ck_dev_buf<double> d_world;               // [4 * n_tags_total][3]
    ck_dev_buf<double> d_bear;                // the call's bearings
    ck_dev_buf<double> d_mounts;              // [n_problems][CK_RIG_MAX_CAMS][12] starts in, results out
    ck_dev_buf<double> d_steps;               // [used steps of the call][CKA_S_STRIDE]; the start poses in, the results out (CKA_S_POSE)
    ck_dev_buf<double> d_views;               // [views of the call][CKA_B_STRIDE]
    ck_dev_buf<ck_rigcal_result_t> d_res;     // [n_problems] starts in (ck_rigcal_result_start), results out
};

// k_rigcal.hip: one workgroup per problem on `stream`; every array is the device's.  d_res[i].status is -1, or CK_CALIB_DEGENERATE:
// the problem is skipped.
int ck_launch_rigcal(hipStream_t stream, int max_iters, int n_cams, int n_steps, const ck_rigcal_dev_problem *d_prob, int n_problems,
                     const int32_t *d_tab, const int32_t *d_index, const double *d_world, const double *d_bear, double *d_mounts,
                     double *d_steps, double *d_views, ck_rigcal_result_t *d_res);

#endif
