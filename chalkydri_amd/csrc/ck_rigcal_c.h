/* Mount calibration: what the host twin (ck_rigcal_host.c, plain C) and the device side (ck_rigcal.h, ck_rigcal.hip)
 * share: everything of a call that is decided or converted on the host, written once so that both return the same bytes. */
#ifndef CK_RIGCAL_C_H
#define CK_RIGCAL_C_H

#include "chalkydri_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
/* What the host decides about one problem before anything is solved */
typedef struct ck_rigcal_plan {
    int32_t n_used;                     /* used steps */
    int32_t n_points;                   /* of the used steps */
    int32_t cam_points[CK_RIG_MAX_CAMS];
    uint64_t mask;                      /* fixed_mask, and all six bits of every camera without a point in the used steps */
    int32_t status;                     /* -1: to be solved; CK_CALIB_DEGENERATE */
    int32_t n_views;                    /* (used step, camera) pairs with points: the blocks of the index */
} ck_rigcal_plan_t;
/* Internal (not part of the C ABI in chalkydri_hip.h).  The arrays are the host's and have passed ck_rigcal_check. */
/* the capture's view table tab[n_cams * n_steps][3] (first world point, first bearing, points) and the tags' corners world[4 * n_tags_total][3] */
void ck_rigcal_table(int32_t n_cams, const ck_sqpnp_problem_t *records, int32_t n_steps, const ck_iso3_t *tags, int32_t n_tags_total,
                     int32_t *tab, double *world);
/* the plan of one problem and its arrowhead index (ck_cal_math.h: cka_index_at(index, n_used, n_views), columns = cameras, blocks =
 * views); index has room for cka_index_size(problem->n_steps, n_cams * problem->n_steps, n_cams); poses0 [n_steps][12] */
void ck_rigcal_plan(const ck_rigcal_params_t *p, int32_t n_cams, const int32_t *tab, int32_t n_steps, const ck_rigcal_problem_t *problem,
                    const int32_t *step_index, const double *poses0, int32_t *index, ck_rigcal_plan_t *plan);
/* robot_to_cam (A, b) <-> the solver's mount M[12] = (A row-major, o = -A^T b) */
void ck_rigcal_mount_in(const ck_iso3_t *iso, double *M);
/* R row-major -> the unit quaternion (w, x, y, z) with w >= 0, by the largest of the four squared components */
void ck_rigcal_mat_to_quat(const double R[9], double q[4]);
/* the result record before the solve (everything but status, iters, the costs and the rms) and after it (robot_to_cam from the
 * solved mounts M[n_cams][12]; frozen parts are mounts0's) */
void ck_rigcal_result_start(const ck_rigcal_problem_t *problem, const ck_rigcal_plan_t *plan, int32_t n_cams, const ck_iso3_t *mounts0,
                            ck_rigcal_result_t *res);
void ck_rigcal_result_finish(const ck_rigcal_plan_t *plan, int32_t n_cams, const ck_iso3_t *mounts0, const double *M, ck_rigcal_result_t *res);
#ifdef __cplusplus
}
#endif

#endif
