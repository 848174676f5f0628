// k_calib.hip — Levenberg-Marquardt refinement of camera intrinsics and board poses: one persistent workgroup of
// 256 threads per problem, the whole iteration inside the kernel.  The arithmetic is ck_calib_math.h's, the same text the host twin
// (ck_calib_host.c) compiles; this file only decides who computes what:
//   observations   a wave takes the frames wave, wave + 4, ...; lane l the observations l, l + 64, ... of the frame; the 64 partial
//                  sums meet in the xor butterfly 32 .. 1, which stands OUTSIDE the lanes' loops: every lane is active at every
//                  exchange (a lane exchange inside a divergent block reads lanes that are switched off; DESIGN.md §5, k_tail)
//   frame records  lane 0 writes the frame's sums into its record (global memory: the records outlive the rejected steps that reuse
//                  them); thread j adds entry j of all records in frame order into LDS
//   6 x 6 solves   thread t takes the frames t, t + 256, ... (one wave for up to 64 frames), all in registers
//   9 x 9 solve    thread 0, on LDS
// The kernel is a template over the camera model (k_calib_impl.h; ck_calib_math.h: OpenCVModel5, or EUCM with UCM as EUCM with slot 5
// frozen): only the residual and the Jacobian of one observation differ, everything that walks, sums and solves is the same text.
// This file instantiates OpenCVModel5, k_calib_eucm.hip the other.
// Plain C++ and __shfl_xor only.
#include "k_calib_impl.h"

int ck_launch_calib(hipStream_t stream, int model, const ck_calib_params_t &p, const ck_calib_problem_t *d_prob, const int32_t *d_rec0, int n_problems,
                    const int32_t *d_fs, const double *d_bxy, const double *d_uv, double *d_rec, double *d_poses, ck_calib_result_t *d_res) {
    if (model != CK_CAMERA_OPENCV5) return ck_launch_calib_eucm(stream, model, p, d_prob, d_rec0, n_problems, d_fs, d_bxy, d_uv, d_rec, d_poses, d_res);
    return launch_calib_model<CKC_MODEL_OPENCV5>(stream, p, d_prob, d_rec0, n_problems, d_fs, d_bxy, d_uv, d_rec, d_poses, d_res);
}
