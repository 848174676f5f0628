// Mount and field calibration: what the two device drivers (ck_rigcal.hip, ck_fieldcal.hip) share besides
// ck_cal_c.h: the starts of ck_rig_calibrate_batch and ck_field_calibrate_batch.
#ifndef CK_CAL_H
#define CK_CAL_H

#include <string.h>

#include <vector>

#include "ck_cal_c.h"
#include "ck_grow.h"

// The caller's problems without the steps that have no start, and where their poses go back to
struct ck_cal_starts {
    std::vector<ck_rigcal_problem_t> prob; // [n]
    std::vector<int32_t> index, where;     // prob's step_index; where[k] = the place of index[k] in the caller's step_index
    std::vector<double> poses0, poses;     // the starts [n_steps][12]; what the refinement returns [where.size()][12]
    int32_t n_index() const { return (int32_t)where.size(); }
};
// The starts (ck_rigcal.hip): the rig solver with `tags` and `mounts` and no gyro penalty over the whole capture, once; its poses
// turned into world -> robot; a step without a pose is left out of every problem.  CK_OK, CK_ENOMEM or the rig solver's code.
int ck_cal_starts_solve(ck_handle_t *h, int32_t n_cams, const ck_sqpnp_problem_t *records, int32_t n_steps, const ck_iso3_t *tags,
                        int32_t n_tags_total, const double *bearings, int32_t n_bearings_total, const double *gyro,
                        const ck_rigcal_problem_t *problems, int32_t n, const int32_t *step_index, const ck_iso3_t *mounts, ck_cal_starts &s);
// After the refinement of s.prob: n_steps as the caller counts them, the poses at the caller's places, zero where a step had no start
template <typename R>
static inline void ck_cal_starts_finish(const ck_cal_starts &s, const ck_rigcal_problem_t *problems, int32_t n, R *results, double *poses_out) {
    for (int32_t i = 0; i < n; i++) {
        results[i].n_steps = problems[i].n_steps;
        memset(poses_out + 12 * (size_t)problems[i].step_offset, 0, sizeof(double) * 12 * (size_t)problems[i].n_steps);
    }
    for (size_t k = 0; k < s.where.size(); k++) memcpy(poses_out + 12 * (size_t)s.where[k], s.poses.data() + 12 * k, sizeof(double) * 12);
}

#endif
