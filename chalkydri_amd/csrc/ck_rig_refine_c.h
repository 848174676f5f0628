/* Rig pose refinement: what the host twin (ck_rig_refine_host.c, plain C) and the device side (ck_rig_refine.h,
 * k_rig_refine.hip) share. */
#ifndef CK_RIG_REFINE_C_H
#define CK_RIG_REFINE_C_H

#include "ck_rig_c.h"

#define CKF_PT 19 /* doubles of a point record in the workspace (ck_rig_refine_math.h) */

#ifdef __cplusplus
extern "C" {
#endif
/* Internal (not part of the C ABI): the refusals of the parameters alone, and ck_rig_refine_host's whole list in its order, with the
 * largest number of points of an instant.  The records lie in host memory; the other pointers are only compared with null. */
int ck_rig_refine_params_check(const ck_rig_refine_params_t *params);
int ck_rig_refine_check(const ck_rig_refine_params_t *params, int32_t n_cams, const ck_sqpnp_problem_t *problems, int32_t n, const void *tags,
                        int32_t n_tags_total, const void *bearings, int32_t n_bearings_total, const void *gyro, const void *start,
                        const void *out, int32_t *max_points);
#ifdef __cplusplus
}
#endif

#endif
