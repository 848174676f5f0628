// ck_mat3.h — fp64 3x3 helpers and the OpenCV-5 undistortion shared by the pose kernels (k_sqpnp.hip, k_tagpose.hip).
// Row-major 3x3 matrices.  Every array is indexed by compile-time constants once the loops are unrolled: a runtime-indexed
// local array lives in scratch memory (DESIGN.md §Per-tag pose: scratch budget).
#ifndef CK_MAT3_H
#define CK_MAT3_H

#include <math.h>

#include "chalkydri_hip.h"
#include "ck_camera_math.h"

static __device__ inline void mat3_mul(const double A[9], const double B[9], double C[9]) {
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) C[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
}
static __device__ inline void mat3_vec(const double A[9], const double v[3], double o[3]) {
    for (int i = 0; i < 3; i++) o[i] = A[i * 3] * v[0] + A[i * 3 + 1] * v[1] + A[i * 3 + 2] * v[2];
}
static __device__ inline double mat3_det(const double m[9]) {
    return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}
static __device__ inline int mat3_try_inverse(const double m[9], double o[9]) {
    double det = mat3_det(m);
    if (det == 0.0) return 0;
    o[0] = (m[4] * m[8] - m[5] * m[7]) / det; o[1] = (m[2] * m[7] - m[1] * m[8]) / det; o[2] = (m[1] * m[5] - m[2] * m[4]) / det;
    o[3] = (m[5] * m[6] - m[3] * m[8]) / det; o[4] = (m[0] * m[8] - m[2] * m[6]) / det; o[5] = (m[2] * m[3] - m[0] * m[5]) / det;
    o[6] = (m[3] * m[7] - m[4] * m[6]) / det; o[7] = (m[1] * m[6] - m[0] * m[7]) / det; o[8] = (m[0] * m[4] - m[1] * m[3]) / det;
    return 1;
}
// serial cyclic Jacobi for small symmetric matrices (used for the 3x3 cases)
static __device__ inline void jacobi3(double A[9], double V[9], double w[3]) {
    for (int i = 0; i < 9; i++) V[i] = (i % 4 == 0);
    double tot = 0; // same stop rule and summation order as the oracle's jacobi_eigen
    for (int i = 0; i < 9; i++) tot += A[i] * A[i];
    const double stop = 1e-32 * tot;
    for (int sweep = 0; sweep < 64; sweep++) {
        double off = 0;
        off += A[1] * A[1]; off += A[2] * A[2]; off += A[5] * A[5];
        if (off <= stop) break;
        for (int p = 0; p < 3; p++)
            for (int q = p + 1; q < 3; q++) {
                double apq = A[p * 3 + q];
                if (fabs(apq) < 1e-300) continue;
                double app = A[p * 3 + p], aqq = A[q * 3 + q];
                double theta = (aqq - app) / (2.0 * apq);
                double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 3; k++) { double akp = A[k * 3 + p], akq = A[k * 3 + q]; A[k * 3 + p] = c * akp - s * akq; A[k * 3 + q] = s * akp + c * akq; }
                for (int k = 0; k < 3; k++) { double apk = A[p * 3 + k], aqk = A[q * 3 + k]; A[p * 3 + k] = c * apk - s * aqk; A[q * 3 + k] = s * apk + c * aqk; }
                for (int k = 0; k < 3; k++) { double vkp = V[k * 3 + p], vkq = V[k * 3 + q]; V[k * 3 + p] = c * vkp - s * vkq; V[k * 3 + q] = s * vkp + c * vkq; }
            }
    }
    for (int i = 0; i < 3; i++) w[i] = A[i * 3 + i];
}
// element k (0..2, a runtime value) of a 3-vector, by selects: no runtime-indexed local array
static __device__ inline double sel3(const double v[3], int k) { return k == 0 ? v[0] : (k == 1 ? v[1] : v[2]); }
static __device__ inline void svd3(const double M[9], double U[9], double s[3], double V[9]) {
    double MtM[9], Vt[9], w[3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) MtM[i * 3 + j] = M[0 + i] * M[0 + j] + M[3 + i] * M[3 + j] + M[6 + i] * M[6 + j];
    jacobi3(MtM, Vt, w);
    // descending order of the eigenvalues: the exchange sort over (0,1), (0,2), (1,2) written out on three scalars
    int i0 = 0, i1 = 1, i2 = 2, tmp;
    if (sel3(w, i1) > sel3(w, i0)) { tmp = i0; i0 = i1; i1 = tmp; }
    if (sel3(w, i2) > sel3(w, i0)) { tmp = i0; i0 = i2; i2 = tmp; }
    if (sel3(w, i2) > sel3(w, i1)) { tmp = i1; i1 = i2; i2 = tmp; }
    for (int c = 0; c < 3; c++) {
        const int ic = c == 0 ? i0 : (c == 1 ? i1 : i2);
        const double wc = sel3(w, ic);
        s[c] = sqrt(wc > 0 ? wc : 0);
        for (int r = 0; r < 3; r++) { const double row[3] = {Vt[r * 3], Vt[r * 3 + 1], Vt[r * 3 + 2]}; V[r * 3 + c] = sel3(row, ic); }
    }
    for (int c = 0; c < 3; c++) {
        double v[3] = {V[c], V[3 + c], V[6 + c]}, u[3];
        mat3_vec(M, v, u);
        double n = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
        if (n > 1e-12 * (s[0] > 0 ? s[0] : 1.0)) { for (int r = 0; r < 3; r++) U[r * 3 + c] = u[r] / n; }
        else if (c == 2) { /* complete a right-handed frame */
            double ua[3] = {U[0], U[3], U[6]}, ub[3] = {U[1], U[4], U[7]};
            double cr[3] = {ua[1] * ub[2] - ua[2] * ub[1], ua[2] * ub[0] - ua[0] * ub[2], ua[0] * ub[1] - ua[1] * ub[0]};
            double cn = sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]);
            for (int r = 0; r < 3; r++) U[r * 3 + 2] = cn > 0 ? cr[r] / cn : (r == 2);
        } else if (c == 1) { /* rank 1: the coordinate axis least aligned with u0 (first on ties), made orthogonal to u0 */
            double u0[3] = {U[0], U[3], U[6]};
            int k = 0;
            for (int r = 1; r < 3; r++)
                if (fabs(u0[r]) < fabs(sel3(u0, k))) k = r;
            const double e[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
            double d = sel3(u0, k), g[3] = {e[0] - d * u0[0], e[1] - d * u0[1], e[2] - d * u0[2]};
            double gn = sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
            for (int r = 0; r < 3; r++) U[r * 3 + 1] = g[r] / gn;
        } else { /* zero matrix: U = I */
            for (int r = 0; r < 3; r++) U[r * 3 + 0] = (r == 0);
        }
    }
}
// nearest rotation of a row-major 3x3 (U V^T with the chirality fix)
static __device__ inline void polar_rotation(const double M[9], double out[9]) {
    double U[9], s[3], V[9], Vt[9];
    svd3(M, U, s, V);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) Vt[i * 3 + j] = V[j * 3 + i];
    mat3_mul(U, Vt, out);
    if (mat3_det(out) < 0.0) {
        for (int r = 0; r < 3; r++) U[r * 3 + 2] = -U[r * 3 + 2];
        mat3_mul(U, Vt, out);
    }
}

// OpenCVModel5 undistortion of one pixel to the normalised point (x, y): the fixed-point iteration of the reference's
// unproject.  With all-zero distortion the first step returns ((u - cx) / fx, (v - cy) / fy) exactly and converges.
static __device__ inline bool undistort_one(const ck_opencv5_t &c, double u, double v, double *xo, double *yo) {
    double xd = (u - c.cx) / c.fx, yd = (v - c.cy) / c.fy;
    double x = xd, y = yd;
    bool conv = false;
    for (int it = 0; it < 50; it++) {
        double r2 = x * x + y * y;
        double radial = 1.0 + r2 * (c.k1 + r2 * (c.k2 + r2 * c.k3));
        double dx = 2.0 * c.p1 * x * y + c.p2 * (r2 + 2.0 * x * x);
        double dy = c.p1 * (r2 + 2.0 * y * y) + 2.0 * c.p2 * x * y;
        double nx = (xd - dx) / radial, ny = (yd - dy) / radial;
        double ex = nx - x, ey = ny - y;
        x = nx; y = ny;
        if (ex * ex + ey * ey < 1e-24) { conv = true; break; }
    }
    *xo = x; *yo = y;
    return conv && isfinite(x) && isfinite(y);
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
