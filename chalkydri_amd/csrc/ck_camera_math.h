// ck_camera_math.h — the arithmetic of the camera models, written once and compiled twice, as ck_calib_math.h is: as
// C into the host functions (ck_camera_host.c) and as device code into the kernels that turn pixels into bearings (k_sqpnp.hip:
// k_camera_unproject, k_glue) and into normalised points (k_tagpose.hip).  Only + - * / sqrt on doubles, every expression evaluated as
// written (-ffp-contract=off on both sides), so the two produce the same bytes.  THE OPERATION ORDER IS PART OF THE CONTRACT.
//
// k[9]: EUCM fx fy cx cy alpha beta 0 0 0.  UCM is EUCM with beta = 1: whoever calls these functions has put 1.0 into k[5]
// (ckm_effective).  OPENCV5: fx fy cx cy k1 k2 p1 p2 k3.
#ifndef CK_CAMERA_MATH_H
#define CK_CAMERA_MATH_H

#include <math.h>

#if defined(__HIPCC__)
#define CKM_FN static __device__ __host__ __forceinline__
#else
#define CKM_FN static inline
#endif

CKM_FN int ckm_finite(double x) { return x - x == 0.0; }

// UCM reads k[5] as 1.0 whatever it holds; models 1 (EUCM) and 2 (UCM) are one code path after this
CKM_FN void ckm_effective(int model, const double *k, double *ke) {
    for (int i = 0; i < 9; i++) ke[i] = k[i];
    if (model == 2) ke[5] = 1.0;
}

// EUCM unprojection of pixel (u, v): (mx, my, kz) is a point on the ray, not yet of unit length.  0: outside the valid disc.
// With alpha = 0: g = 1, kz = (1 - 0) / (0 + 1) = 1.0 exactly, and (mx, my) are OpenCVModel5's first fixed-point step.
CKM_FN int ckm_eucm_ray(const double *k, double u, double v, double *mx_o, double *my_o, double *kz_o) {
    const double alpha = k[4], beta = k[5];
    const double mx = (u - k[2]) / k[0], my = (v - k[3]) / k[1];
    const double r2 = mx * mx + my * my;
    const double g = 1.0 - alpha;
    *mx_o = mx; *my_o = my; *kz_o = 0.0;
    if (alpha > 0.5 && !(r2 < 1.0 / (beta * (alpha - g)))) return 0;
    const double s = sqrt(1.0 - ((alpha - g) * beta) * r2);
    *kz_o = (1.0 - ((alpha * alpha) * beta) * r2) / (alpha * s + g);
    return 1;
}
// ... as a unit bearing.  b is written in every case (zeros outside the disc); 1: inside the disc and all finite
CKM_FN int ckm_eucm_unproject(const double *k, double u, double v, double *b) {
    double mx, my, kz;
    if (!ckm_eucm_ray(k, u, v, &mx, &my, &kz)) { b[0] = 0.0; b[1] = 0.0; b[2] = 0.0; return 0; }
    const double nrm = sqrt(mx * mx + my * my + kz * kz);
    b[0] = mx / nrm; b[1] = my / nrm; b[2] = kz / nrm;
    return ckm_finite(b[0]) && ckm_finite(b[1]) && ckm_finite(b[2]);
}
// ... as the normalised point (x, y, 1) of the per-tag pose: additionally kz > 0.  (x, y) = (0, 0) when there is none.
CKM_FN int ckm_eucm_normalize(const double *k, double u, double v, double *x, double *y) {
    double mx, my, kz;
    *x = 0.0; *y = 0.0;
    if (!ckm_eucm_ray(k, u, v, &mx, &my, &kz)) return 0;
    if (!(kz > 0.0)) return 0;
    *x = mx / kz; *y = my / kz;
    return ckm_finite(*x) && ckm_finite(*y);
}

// EUCM projection of the camera point (X, Y, Z).  0: not valid (den <= 0 or behind the cone Z > -w d); the pixel is (0, 0) then.
CKM_FN int ckm_eucm_project(const double *k, double X, double Y, double Z, double *u, double *v) {
    const double alpha = k[4], beta = k[5];
    const double d = sqrt(beta * (X * X + Y * Y) + Z * Z);
    const double den = alpha * d + (1.0 - alpha) * Z;
    const double w = alpha > 0.5 ? (1.0 - alpha) / alpha : alpha / (1.0 - alpha);
    *u = 0.0; *v = 0.0;
    if (!(den > 0.0) || !(Z > -w * d)) return 0;
    const double pu = k[0] * (X / den) + k[2], pv = k[1] * (Y / den) + k[3];
    if (!ckm_finite(pu) || !ckm_finite(pv)) return 0;
    *u = pu; *v = pv;
    return 1;
}

// OpenCVModel5 undistortion of one pixel to the normalised point (x, y): the fixed-point iteration of the reference's unproject.
// With all-zero distortion the first step returns ((u - cx) / fx, (v - cy) / fy) exactly and converges.
CKM_FN int ckm_opencv5_undistort(const double *c, double u, double v, double *xo, double *yo) {
    const double xd = (u - c[2]) / c[0], yd = (v - c[3]) / c[1];
    double x = xd, y = yd;
    int conv = 0;
    for (int it = 0; it < 50; it++) {
        const double r2 = x * x + y * y;
        const double radial = 1.0 + r2 * (c[4] + r2 * (c[5] + r2 * c[8]));
        const double dx = 2.0 * c[6] * x * y + c[7] * (r2 + 2.0 * x * x);
        const double dy = c[6] * (r2 + 2.0 * y * y) + 2.0 * c[7] * x * y;
        const double nx = (xd - dx) / radial, ny = (yd - dy) / radial;
        const double ex = nx - x, ey = ny - y;
        x = nx; y = ny;
        if (ex * ex + ey * ey < 1e-24) { conv = 1; break; }
    }
    *xo = x; *yo = y;
    return conv && ckm_finite(x) && ckm_finite(y);
}
CKM_FN int ckm_opencv5_unproject(const double *c, double u, double v, double *b) {
    double x, y;
    const int ok = ckm_opencv5_undistort(c, u, v, &x, &y);
    const double nrm = sqrt(x * x + y * y + 1.0);
    b[0] = x / nrm; b[1] = y / nrm; b[2] = 1.0 / nrm;
    return ok;
}
// OpenCVModel5 projection (the distortion of ck_calib_math.h's ckc_residual)
CKM_FN int ckm_opencv5_project(const double *c, double X, double Y, double Z, double *u, double *v) {
    *u = 0.0; *v = 0.0;
    if (!(Z > 0.0)) return 0;
    const double x = X / Z, y = Y / Z;
    const double r2 = x * x + y * y;
    const double rad = 1.0 + r2 * (c[4] + r2 * (c[5] + r2 * c[8]));
    const double xy2 = (2.0 * x) * y;
    const double xd = x * rad + c[6] * xy2 + c[7] * (r2 + (2.0 * x) * x);
    const double yd = y * rad + c[6] * (r2 + (2.0 * y) * y) + c[7] * xy2;
    const double pu = c[0] * xd + c[2], pv = c[1] * yd + c[3];
    if (!ckm_finite(pu) || !ckm_finite(pv)) return 0;
    *u = pu; *v = pv;
    return 1;
}

#endif
