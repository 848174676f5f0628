// Camera rig: what k_rigpnp.hip (kernel and entry points) and the handle (ck_api.hip) share; ck_rig_c.h is the part the
// host twin (plain C) shares too.
#ifndef CK_RIG_H
#define CK_RIG_H

#include "ck_grow.h"
#include "ck_rig_c.h"

#define CK_RIG_POINT_DOUBLES 7 // per point of the first pass: world point [3], ray direction in the robot frame [3], camera index

// Workspace, allocated by the first rig call and grown on demand (ck_create allocates none of it)
struct ck_rig_ws {
    ck_dev_buf<double> d_points;            // [n][max_points][CK_RIG_POINT_DOUBLES] the kernel's first pass
    ck_dev_buf<ck_rig_result_t> d_res;      // [n]
    ck_dev_buf<ck_rig_robust_result_t> d_rres; // [n] the robust calls' records, in d_res's place
    ck_dev_buf<double> d_gyro;              // [n]
    ck_dev_buf<uint8_t> d_has_gyro;         // [n] (ck_rig_process_last)
    ck_dev_buf<ck_vision_measurement_t> d_meas; // [n]
    ck_dev_buf<int32_t> d_valid;            // [n]
    ck_dev_buf<ck_sqpnp_problem_t> d_prob;  // [n_cams][n] the inputs of ck_rig_solve_batch
    ck_dev_buf<ck_iso3_t> d_tags;
    ck_dev_buf<double> d_bearings;
    hipEvent_t ev[CK_RIG_MAX_CAMS] = {};    // ck_rig_process_last: "camera c's records are complete", recorded on its handle's stream
    ~ck_rig_ws() { for (auto &e : ev) if (e) (void)hipEventDestroy(e); }
};

// k_rigpnp.hip, for ck_rig_refine.hip: everything ck_rig_process_last (rp null) or ck_rig_process_last_robust (params = &rp->rig, out a
// ck_rig_robust_result_t[n]) enqueues on handles[0]'s stream, without the wait; and k_rig once more over what the last
// ck_rig_solve_batch of this shape left in the workspace (a measurement aid)
int ck_rig_enqueue_last(ck_handle_t *const *handles, int32_t n_cams, int32_t n, const ck_rig_params_t *params,
                        const ck_rig_robust_params_t *rp, const double *gyro, const uint8_t *has_gyro, void *out,
                        ck_vision_measurement_t *meas, int32_t *valid);
int ck_rig_relaunch_batch(ck_handle_t *h, const ck_rig_params_t *params, int32_t n_cams, int32_t n, int32_t max_points);

#endif
