// Field calibration: what ck_fieldcal.hip (host) and k_fieldcal.hip (kernel) share; ck_fieldcal_c.h is the part the
// host twin (plain C) shares too.
#ifndef CK_FIELDCAL_H
#define CK_FIELDCAL_H

#include "ck_fieldcal_c.h"
#include "ck_grow.h"

// One problem as the kernel sees it: where its tables and records start in the call's buffers, and their sizes
struct ck_fieldcal_dev_problem {
    int64_t meta_off;  // int32 entries into d_meta (ckf_meta_at over U, P, NS, T)
    int64_t step_off;  // records into d_steps
    int64_t pair_off;  // records into d_pairs
    int64_t sight_off; // records into d_sights
    int64_t s_off;     // doubles into d_S: the packed lower triangle of its 6 T x 6 T reduced system
    int32_t U, P, NS, T;
};

// Workspace, allocated by the first field calibration call and grown on demand (ck_create allocates none of it)
struct ck_fieldcal_ws {
    ck_dev_buf<ck_fieldcal_dev_problem> d_prob; // [n_problems]
    ck_dev_buf<int32_t> d_meta;                 // the problems' integer tables
    ck_dev_buf<double> d_bear;                  // the call's bearings
    ck_dev_buf<double> d_mounts;                // [n_cams][12]
    ck_dev_buf<double> d_tags;                  // [n_problems][CK_FIELDCAL_MAX_TAGS][12] starts in, results out
    ck_dev_buf<double> d_rms;                   // [n_problems][CK_FIELDCAL_MAX_TAGS] the tags' rms out
    ck_dev_buf<double> d_steps;                 // [used steps of the call][CKA_S_STRIDE]; the start poses in, the results out (CKA_S_POSE)
    ck_dev_buf<double> d_pairs;                 // [pairs of the call][CKA_B_STRIDE]
    ck_dev_buf<double> d_sights;                // [sightings of the call][CKF_I_STRIDE]
    ck_dev_buf<double> d_S;                     // the problems' reduced systems
    ck_dev_buf<ck_fieldcal_result_t> d_res;     // [n_problems] starts in (ck_fieldcal_result_start), results out
};

// k_fieldcal.hip: one workgroup per problem on `stream`; every array is the device's.  d_res[i].status is -1, or CK_CALIB_DEGENERATE:
// the problem is skipped.
int ck_launch_fieldcal(hipStream_t stream, int max_iters, int n_cams, const ck_fieldcal_dev_problem *d_prob, int n_problems, const int32_t *d_meta,
                       const double *d_bear, const double *d_mounts, double *d_tags, double *d_rms, double *d_steps, double *d_pairs,
                       double *d_sights, double *d_S, ck_fieldcal_result_t *d_res);

#endif
