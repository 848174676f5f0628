// Camera calibration: what ck_calib.hip (host) and k_calib.hip (kernel) share.
#ifndef CK_CALIB_H
#define CK_CALIB_H

#include "ck_grow.h"

// Workspace, allocated by the first calibration call and grown on demand (ck_create allocates none of it)
struct ck_calib_ws {
    ck_dev_buf<ck_calib_problem_t> d_prob; // [n_problems]
    ck_dev_buf<int32_t> d_rec0;            // [n_problems] first frame record of each problem in d_rec
    ck_dev_buf<int32_t> d_fs;              // the call's frame_start
    ck_dev_buf<double> d_bxy, d_uv;        // the call's points
    ck_dev_buf<double> d_rec;              // [frames of the call][CKC_WS_STRIDE] the frame records (ck_calib_math.h)
    ck_dev_buf<double> d_poses;            // [n_frames_total][12] starts in, results out
    ck_dev_buf<ck_calib_result_t> d_res;   // [n_problems] starts in (cam, status), results out
};

extern "C" int ck_calib_start_ok(const double *cam0, const double *poses, int n_frames); // ck_calib_host.c: a start the solver can take

// ck_calib_host.c: the solver's record (any model's parameters in the nine slots of .cam) <-> the camera-model entry points' types
extern "C" void ck_calib_result_to_camera(int model, const ck_calib_result_t *r, int start, int n_starts, ck_camera_calib_result_t *o);
extern "C" void ck_calib_start_from_camera(int model, const ck_camera_t *cam, ck_opencv5_t *k0);

// k_calib.hip: one workgroup per problem on `stream`; every array is the device's.  d_res[i] holds the start (cam, n_frames,
// n_points, status -1, or CK_CALIB_DEGENERATE: the problem is skipped), d_poses the start poses.  model: CK_CAMERA_*; an EUCM / UCM
// problem keeps its six parameters in the nine slots of ck_calib_result_t.cam (ck_calib_math.h).
int ck_launch_calib(hipStream_t stream, int model, const ck_calib_params_t &p, const ck_calib_problem_t *d_prob, const int32_t *d_rec0, int n_problems,
                    const int32_t *d_fs, const double *d_bxy, const double *d_uv, double *d_rec, double *d_poses, ck_calib_result_t *d_res);
// k_calib_eucm.hip: the same for CK_CAMERA_EUCM / CK_CAMERA_UCM (ck_launch_calib forwards here)
int ck_launch_calib_eucm(hipStream_t stream, int model, const ck_calib_params_t &p, const ck_calib_problem_t *d_prob, const int32_t *d_rec0,
                         int n_problems, const int32_t *d_fs, const double *d_bxy, const double *d_uv, double *d_rec, double *d_poses,
                         ck_calib_result_t *d_res);

#endif
