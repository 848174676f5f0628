// Rig pose refinement: what ck_rig_refine.hip (entry points) and k_rig_refine.hip (kernel) share; ck_rig_refine_c.h is the
// part the host twin (plain C) shares too.
#ifndef CK_RIG_REFINE_H
#define CK_RIG_REFINE_H

#include "ck_grow.h"
#include "ck_rig_refine_c.h"

// One camera's arrays as the kernel reads them (k_rigpnp.hip's RigCam without the counters)
struct ck_rig_refine_cam {
    const ck_sqpnp_problem_t *problems; // [n] this camera's record of every instant
    const ck_iso3_t *tags;
    const double *bearings;
    int det_cap;                        // > 0: a handle's workspace, instant s owns tags[s * det_cap ..] and bearings[s * det_cap * 4 ..]; 0: the records' offsets
    int pad;
};
struct ck_rig_refine_args {
    ck_rig_refine_params_t prm;
    ck_rig_refine_cam cam[CK_RIG_MAX_CAMS];
    int n_cams, n;
    int max_points;                     // capacity of an instant in `pts`
    int device_heading;                 // 0: gyro = [n][2] cosine and sine; 1: gyro = [n] headings, cosine and sine taken by the kernel
    const double *gyro;                 // null without the prior
    const char *start;                  // the fused records: a ck_rig_result_t every start_stride bytes
    size_t start_stride;
    const uint64_t *rejected;           // [CK_RIG_MAX_CAMS] masks every rejected_stride words, or null
    size_t rejected_stride;
    double *pts;                        // [n][CKF_PT][max_points]
    ck_rig_refined_t *out;              // [n]
    ck_vision_measurement_t *meas;      // [n] or null: the fused measurements, which take the refined pose where there is one
};

// Workspace, allocated by the first refinement call and grown on demand (ck_create allocates none of it)
struct ck_rig_refine_ws {
    ck_dev_buf<double> d_pts;
    ck_dev_buf<ck_rig_refined_t> d_out;
    ck_dev_buf<double> d_gyro;
    ck_dev_buf<ck_rig_result_t> d_start;
    ck_dev_buf<uint64_t> d_rejected;
    ck_dev_buf<ck_sqpnp_problem_t> d_prob;
    ck_dev_buf<ck_iso3_t> d_tags;
    ck_dev_buf<double> d_bearings;
};

// k_rig_refine.hip: one wave per instant on `stream`; every array is the device's
int ck_launch_rig_refine(hipStream_t stream, const ck_rig_refine_args &a);

#endif
