/* Camera rig: what the host twin (ck_rig_host.c, plain C) and the device side (ck_rig.h, k_rigpnp.hip) share. */
#ifndef CK_RIG_C_H
#define CK_RIG_C_H

#include "chalkydri_hip.h"

/* smallest / largest eigenvalue of the scatter of the centred points at or below it: the points are coplanar, and the starts are
 * taken outside Omega's exact null space ("Starts on coplanar points") */
#define CK_RIG_PLANAR_EPS 1e-12

#ifdef __cplusplus
extern "C" {
#endif
/* Internal (not part of the C ABI in chalkydri_hip.h): what both solvers refuse, ck_rig_solve_host's list, and the largest number of
 * points of a step.  The records lie in host memory; the other pointers are only compared with null. */
int ck_rig_check(const ck_rig_params_t *params, int32_t n_cams, const ck_sqpnp_problem_t *problems, int32_t n, const void *tags,
                 int32_t n_tags_total, const void *bearings, int32_t n_bearings_total, const void *gyro, const void *out,
                 int32_t *max_points);
/* ... and what the robust solvers refuse beyond that: the four parameters of the robust params and, when `problems` (host
 * memory, already through ck_rig_check) is given, a record of more than CK_RIG_ROBUST_MAX_TAGS tags. */
int ck_rig_robust_check(const ck_rig_robust_params_t *params, int32_t n_cams, const ck_sqpnp_problem_t *problems, int32_t n);
#ifdef __cplusplus
}
#endif

#endif
