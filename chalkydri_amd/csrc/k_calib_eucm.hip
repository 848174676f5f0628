// k_calib_eucm.hip — the EUCM / UCM instantiation of the calibration kernel (k_calib_impl.h): one workgroup of 256
// threads per problem, the summation order of ck_calib_math.h.  UCM runs as EUCM with slot 5 frozen at the 1.0 its start holds.
#include "k_calib_impl.h"

int ck_launch_calib_eucm(hipStream_t stream, int model, const ck_calib_params_t &p, const ck_calib_problem_t *d_prob, const int32_t *d_rec0,
                         int n_problems, const int32_t *d_fs, const double *d_bxy, const double *d_uv, double *d_rec, double *d_poses,
                         ck_calib_result_t *d_res) {
    ck_calib_params_t q = p;
    q.fixed_mask |= ckc_model_mask(model); // (UCM: slot 5 too)
    return launch_calib_model<CKC_MODEL_EUCM>(stream, q, d_prob, d_rec0, n_problems, d_fs, d_bxy, d_uv, d_rec, d_poses, d_res);
}
