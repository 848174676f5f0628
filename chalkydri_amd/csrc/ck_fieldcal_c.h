/* Field calibration: what the host twin (ck_fieldcal_host.c, plain C) and the device side (ck_fieldcal.h,
 * ck_fieldcal.hip) share: everything of a call that is decided or converted on the host, written once so that both return the same
 * bytes. */
#ifndef CK_FIELDCAL_C_H
#define CK_FIELDCAL_C_H

#include <stddef.h>

#include "chalkydri_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
/* What the host decides about one problem before anything is solved.  meta: the integer tables of ck_fieldcal_math.h (ckf_meta_at over
 * n_used, n_pairs, n_sights, n_tags), malloc'ed; release with ck_fieldcal_plan_free. */
typedef struct ck_fieldcal_plan {
    int32_t status;                /* -1: to be solved; CK_CALIB_DEGENERATE */
    int32_t n_used, n_pairs, n_sights, n_tags;
    int32_t n_points;              /* 4 * n_sights */
    int32_t n_solved;              /* tags with sightings and a free increment */
    int32_t pad;
    int32_t *meta;
    size_t n_meta;                 /* int32 entries of meta */
} ck_fieldcal_plan_t;
/* Internal (not part of the C ABI in chalkydri_hip.h).  The arrays are the host's and have passed ck_fieldcal_check.
 * CK_OK, CK_ENOMEM; tag_sightings [n_layout] is written too. */
int ck_fieldcal_plan(const ck_fieldcal_params_t *p, int32_t n_cams, const ck_sqpnp_problem_t *records, int32_t n_steps,
                     const int32_t *tag_index, const ck_rigcal_problem_t *problem, const int32_t *step_index, int32_t n_layout,
                     const uint8_t *fixed6, const double *poses0, int32_t *tag_sightings, ck_fieldcal_plan_t *plan);
void ck_fieldcal_plan_free(ck_fieldcal_plan_t *plan);
/* a layout entry -> the solver's tag T[12] = (Q row-major, c) */
void ck_fieldcal_tag_in(const ck_iso3_t *iso, double *T);
/* the outputs before the solve (everything but status, iters, the costs and the rms; the layout is layout0, tag_rms zero) and after it
 * (the solved tags T [n_tags][12] and their rms [n_tags] into the layout's entries; frozen parts are layout0's) */
void ck_fieldcal_result_start(const ck_rigcal_problem_t *problem, const ck_fieldcal_plan_t *plan, const ck_iso3_t *layout0, int32_t n_layout,
                              ck_fieldcal_result_t *res, ck_iso3_t *layout_out, double *tag_rms);
void ck_fieldcal_result_finish(const ck_fieldcal_plan_t *plan, const ck_iso3_t *layout0, const double *T, const double *rms,
                               ck_iso3_t *layout_out, double *tag_rms);
#ifdef __cplusplus
}
#endif

#endif
