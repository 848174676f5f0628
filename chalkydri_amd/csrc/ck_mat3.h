// ck_mat3.h — what the pose kernels (k_sqpnp.hip, k_tagpose.hip) share and C cannot say: the undistortion and unprojection of a
// pixel by a ck_opencv5_t or a ck_camera_t.  The 3x3 helpers are ck_pose_math.h's, the camera models ck_camera_math.h's.
#ifndef CK_MAT3_H
#define CK_MAT3_H

#include <math.h>

#include "chalkydri_hip.h"
#include "ck_camera_math.h"
#include "ck_pose_math.h"

// OpenCVModel5 undistortion of one pixel to the normalised point (x, y): ckm_opencv5_undistort on the struct's nine doubles
static __device__ inline bool undistort_one(const ck_opencv5_t &c, double u, double v, double *xo, double *yo) {
    const double k[9] = {c.fx, c.fy, c.cx, c.cy, c.k1, c.k2, c.p1, c.p2, c.k3};
    return ckm_opencv5_undistort(k, u, v, xo, yo) != 0;
}
// ... as a unit bearing (x, y, 1) / |(x, y, 1)|
static __device__ inline bool unproject_one(const ck_opencv5_t &c, double u, double v, double b[3]) {
    double x, y;
    const bool ok = undistort_one(c, u, v, &x, &y);
    double nrm = sqrt(x * x + y * y + 1.0);
    b[0] = x / nrm; b[1] = y / nrm; b[2] = 1.0 / nrm;
    return ok;
}

// The same two for a ck_camera_t (ck_set_camera): OpenCVModel5 takes the two functions above, EUCM / UCM the closed
// form of ck_camera_math.h (the host has put 1.0 into UCM's k[5]).
static __device__ inline ck_opencv5_t opencv5_of(const ck_camera_t &c) {
    return ck_opencv5_t{c.k[0], c.k[1], c.k[2], c.k[3], c.k[4], c.k[5], c.k[6], c.k[7], c.k[8]};
}
static __device__ inline bool camera_undistort_one(const ck_camera_t &c, double u, double v, double *xo, double *yo) {
    if (c.model == CK_CAMERA_OPENCV5) return undistort_one(opencv5_of(c), u, v, xo, yo);
    return ckm_eucm_normalize(c.k, u, v, xo, yo) != 0;
}
static __device__ inline bool camera_unproject_one(const ck_camera_t &c, double u, double v, double b[3]) {
    if (c.model == CK_CAMERA_OPENCV5) return unproject_one(opencv5_of(c), u, v, b);
    return ckm_eucm_unproject(c.k, u, v, b) != 0;
}

#endif
