/* Mount and field calibration: the host code the two share (ck_cal_host.c, plain C), used by both twins and both
 * device drivers. */
#ifndef CK_CAL_C_H
#define CK_CAL_C_H

#include "chalkydri_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
/* every number finite and the quaternion not zero */
int ck_cal_iso_finite(const ck_iso3_t *t);
/* union-find with path halving */
int ck_cal_find(int *parent, int i);
/* What ck_rigcal_check and ck_fieldcal_check both refuse with CK_EINVAL, else CK_OK: null arrays, counts out of range, records that
 * leave their arrays or are not 4 bearings per tag, problems that leave step_index or whose steps do not increase, the three
 * parameters (min_per_step: cameras there, tags here), a bearing or a mount that is not finite.  `tags` is only tested for null. */
int ck_cal_check(int32_t n_cams, const ck_sqpnp_problem_t *records, int32_t n_steps, const void *tags, int32_t n_tags_total,
                 const double *bearings, int32_t n_bearings_total, const ck_rigcal_problem_t *problems, int32_t n_problems,
                 const int32_t *step_index, int32_t n_index_total, const ck_iso3_t *mounts, int32_t max_iters, int32_t min_steps,
                 int32_t min_per_step);
/* poses_out of a problem's steps = their starts (what a skipped step and a DEGENERATE problem return) */
void ck_cal_poses_start(const ck_rigcal_problem_t *problem, const int32_t *step_index, const double *poses0, double *poses_out);
/* the step records (ck_cal_math.h, CKA_S_*) of n_used used steps: accepted and candidate pose = the start */
void ck_cal_steps_seed(double *steps, const int32_t *used, int32_t n_used, const double *poses0);
/* ... and their accepted poses into poses_out, each at its step's place in the problem's run of step_index */
void ck_cal_poses_finish(const ck_rigcal_problem_t *problem, const int32_t *step_index, const int32_t *used, int32_t n_used,
                         const double *steps, double *poses_out);
#ifdef __cplusplus
}
#endif

#endif
