// ck_pose_math.h — the leaf arithmetic of the pose solvers, written once and compiled twice, as ck_camera_math.h
// is: as C into the host twins (ck_rig_host.c, ck_rigcal_host.c, ck_fieldcal_host.c, ck_rig_refine_host.c) and as device code into the
// kernels (k_sqpnp.hip, k_rigpnp.hip, k_tagpose.hip, k_rig_refine.hip).  Only + - * / sqrt on doubles, and cos sin atan2 asin fmod fabs
// of the C library where the yaw pivot needs them; every expression evaluated as written (-ffp-contract=off on both sides), so the two
// sides differ by the round-off of those library calls alone.  THE OPERATION ORDER IS PART OF THE CONTRACT.
//
// Row-major 3x3 matrices.  Every array is indexed by compile-time constants once the loops are unrolled: a runtime-indexed local
// array lives in scratch memory on the device (DESIGN.md §Per-tag pose: scratch budget), hence sel3.
#ifndef CK_POSE_MATH_H
#define CK_POSE_MATH_H

#include <float.h>
#include <math.h>

#if defined(__HIPCC__)
#define CKP_FN static __device__ __host__ inline
#else
#define CKP_FN static inline
#endif

// the constants of the reference's solver (chalkydri_sqpnp/src/lib.rs:29-39)
#define XY_STD_DEV_SCALAR 5.0
#define THETA_STD_DEV_SCALAR 2.0
#define MAX_TRUSTABLE_RMS 0.1
#define MAX_GYRO_DELTA 30.0
#define TAG_SIZE 0.1651
#define CORNER_DISTANCE (TAG_SIZE / 2.0)
#define PI_D 3.14159265358979323846

CKP_FN void quat_to_mat(const double q[4], double R[9]) { // (w, x, y, z) of any length > 0
    double w = q[0], x = q[1], y = q[2], z = q[3];
    double n = sqrt(w * w + x * x + y * y + z * z);
    w /= n; x /= n; y /= n; z /= n;
    R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w);     R[2] = 2 * (x * z + y * w);
    R[3] = 2 * (x * y + z * w);     R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
    R[6] = 2 * (x * z - y * w);     R[7] = 2 * (y * z + x * w);     R[8] = 1 - 2 * (x * x + y * y);
}
CKP_FN void mat3_mul(const double A[9], const double B[9], double C[9]) {
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) C[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
}
CKP_FN void mat3_vec(const double A[9], const double v[3], double o[3]) {
    for (int i = 0; i < 3; i++) o[i] = A[i * 3] * v[0] + A[i * 3 + 1] * v[1] + A[i * 3 + 2] * v[2];
}
CKP_FN double mat3_det(const double m[9]) {
    return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}
CKP_FN int mat3_try_inverse(const double m[9], double o[9]) {
    double det = mat3_det(m);
    if (det == 0.0) return 0;
    o[0] = (m[4] * m[8] - m[5] * m[7]) / det; o[1] = (m[2] * m[7] - m[1] * m[8]) / det; o[2] = (m[1] * m[5] - m[2] * m[4]) / det;
    o[3] = (m[5] * m[6] - m[3] * m[8]) / det; o[4] = (m[0] * m[8] - m[2] * m[6]) / det; o[5] = (m[2] * m[3] - m[0] * m[5]) / det;
    o[6] = (m[3] * m[7] - m[4] * m[6]) / det; o[7] = (m[1] * m[6] - m[0] * m[7]) / det; o[8] = (m[0] * m[4] - m[1] * m[3]) / det;
    return 1;
}
// serial cyclic Jacobi of a symmetric 3x3 (destroyed); the columns of V are the eigenvectors.  Stop rule, sweep order and rotation
// formulas are those of the 9x9 of the pose kernels (jacobi9_wave) and of the oracle's jacobi_eigen.
CKP_FN void jacobi3(double A[9], double V[9], double w[3]) {
    for (int i = 0; i < 9; i++) V[i] = (i % 4 == 0);
    double tot = 0;
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
CKP_FN double sel3(const double v[3], int k) { return k == 0 ? v[0] : (k == 1 ? v[1] : v[2]); }
CKP_FN void svd3(const double M[9], double U[9], double s[3], double V[9]) {
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
CKP_FN void polar_rotation(const double M[9], double out[9]) {
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
CKP_FN void nearest_so3(const double r_vec[9], double out[9]) { // column-major in and out (lib.rs:42-59)
    double M[9], rot[9];
    for (int c = 0; c < 3; c++)
        for (int r = 0; r < 3; r++) M[r * 3 + c] = r_vec[c * 3 + r];
    polar_rotation(M, rot);
    for (int c = 0; c < 3; c++)
        for (int r = 0; r < 3; r++) out[c * 3 + r] = rot[r * 3 + c];
}

// corner 0..3 of the tag at (R, t) in the world: corner_points_from_center (lib.rs:379-394)
CKP_FN void ckp_tag_corner(const double R[9], const double t[3], int corner, double X[3]) {
    const double cp[4][3] = {{0, -CORNER_DISTANCE, -CORNER_DISTANCE}, {0, CORNER_DISTANCE, -CORNER_DISTANCE},
                             {0, CORNER_DISTANCE, CORNER_DISTANCE}, {0, -CORNER_DISTANCE, CORNER_DISTANCE}};
    double p[3];
    mat3_vec(R, cp[corner], p);
    for (int k = 0; k < 3; k++) X[k] = p[k] + t[k];
}
// a camera mounted by robot_to_cam = (A, b): its centre o = -A^T b and the ray u = A^T v of a bearing v, both in the robot frame
CKP_FN void ckp_camera_origin(const double A[9], const double b[3], double o[3]) {
    for (int k = 0; k < 3; k++) o[k] = -(A[k] * b[0] + A[3 + k] * b[1] + A[6 + k] * b[2]);
}
CKP_FN void ckp_ray(const double A[9], const double v[3], double u[3]) {
    for (int k = 0; k < 3; k++) u[k] = A[k] * v[0] + A[3 + k] * v[1] + A[6 + k] * v[2];
}
// The world point X at the pose (R, t) against the ray u through o: d = R X + t - o.  Returns |M d|^2, M = I - u u^T / u^T u, the
// squared point-to-ray distance (d^T M d = |M d|^2, M is a projector: the square of a small vector, not the product of a small with
// a large one); *ud = u . d (> 0: in front of the origin), *dd = |d|^2.
CKP_FN double ckp_ray_residual(const double R[9], const double t[3], const double X[3], const double u[3], const double o[3], double *ud,
                               double *dd) {
    const double sq = u[0] * u[0] + u[1] * u[1] + u[2] * u[2], inv = 1.0 / sq;
    double d[3], Pd[3];
    mat3_vec(R, X, d);
    for (int k = 0; k < 3; k++) d[k] = (d[k] + t[k]) - o[k];
    *ud = u[0] * d[0] + u[1] * d[1] + u[2] * d[2];
    const double along = *ud * inv;
    for (int k = 0; k < 3; k++) Pd[k] = d[k] - u[k] * along;
    *dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    return Pd[0] * Pd[0] + Pd[1] * Pd[1] + Pd[2] * Pd[2];
}
// the weight of a tag of residual rho in a GNC-TLS round of parameter mu, gate c, c2 = c^2
CKP_FN double gnc_weight(double rho, double mu, double c, double c2) {
    const double lo = (mu / (mu + 1.0)) * c2, hi = ((mu + 1.0) / mu) * c2;
    if (rho <= lo) return 1.0;
    if (rho >= hi) return 0.0;
    return (c / sqrt(rho)) * sqrt(mu * (mu + 1.0)) - mu;
}
// R (row-major) of r (column-major) and the t that goes with it: t = Q_tt^-1 (q_t - Q_rt^T r) - R centroid
CKP_FN void ckp_translation(const double *Qrt, const double *qt, const double *QttInv, const double *centroid, const double *r, double Rm[9],
                            double t[3]) {
    for (int c = 0; c < 3; c++)
        for (int rr = 0; rr < 3; rr++) Rm[rr * 3 + c] = r[c * 3 + rr];
    double d[3], tl[3], Rc[3];
    for (int j = 0; j < 3; j++) {
        double s = 0;
        for (int i = 0; i < 9; i++) s += Qrt[i * 3 + j] * r[i];
        d[j] = qt[j] - s;
    }
    mat3_vec(QttInv, d, tl);
    mat3_vec(Rm, centroid, Rc);
    for (int k = 0; k < 3; k++) t[k] = tl[k] - Rc[k];
}
// compute_std_devs (lib.rs:224-246) of n_tags tags at `distance` whose squared residuals sum to `energy`
CKP_FN void ckp_std_devs(double energy, int n_tags, double distance, double out[3]) {
    double n_points = (double)(n_tags * 4);
    double rms = sqrt(energy / n_points);
    if (rms > MAX_TRUSTABLE_RMS) { out[0] = out[1] = out[2] = DBL_MAX; }
    else {
        double mult = 1.0 + (distance / TAG_SIZE);
        double xy = ((rms * mult) / sqrt((double)n_tags)) * XY_STD_DEV_SCALAR;
        xy = xy < 0.01 ? 0.01 : (xy > 10.0 ? 10.0 : xy);
        double th = (((rms / TAG_SIZE) * mult) / sqrt((double)n_tags)) * THETA_STD_DEV_SCALAR;
        th = th < 0.05 ? 0.05 : (th > PI_D ? PI_D : th);
        out[0] = xy; out[1] = xy; out[2] = th;
    }
}
// The yaw pivot (lib.rs:328-376): the robot's pose world <- robot (robot_rot, robot_pos) turned about the vertical through the mean
// tag centre tc towards the gyro's heading, by the whole difference from MAX_GYRO_DELTA degrees on (smoothstep below); the yaw of the result.
CKP_FN void ckp_yaw_pivot(const double robot_rot[9], const double robot_pos[3], const double tc[3], double gyro, double rot[9], double pos[3],
                          double *yaw_out) {
    double vision_yaw = atan2(robot_rot[3], robot_rot[0]);
    double delta_yaw = gyro - vision_yaw;
    delta_yaw = fmod(delta_yaw + PI_D, 2.0 * PI_D);
    if (delta_yaw < 0) delta_yaw += 2.0 * PI_D;
    delta_yaw -= PI_D;
    double delta_deg = fabs(delta_yaw) * (180.0 / PI_D);
    double weight = delta_deg / MAX_GYRO_DELTA;
    weight = weight < 0 ? 0 : (weight > 1 ? 1 : weight);
    weight = weight * weight * (3.0 - 2.0 * weight);
    double applied = delta_yaw * weight;
    double cz = cos(applied), sz = sin(applied);
    double rotz[9] = {cz, -sz, 0, sz, cz, 0, 0, 0, 1};
    double rel[3] = {robot_pos[0] - tc[0], robot_pos[1] - tc[1], robot_pos[2] - tc[2]}, piv[3], R2[9];
    mat3_vec(rotz, rel, piv);
    mat3_mul(rotz, robot_rot, R2);
    for (int k = 0; k < 3; k++) pos[k] = tc[k] + piv[k];
    for (int k = 0; k < 9; k++) rot[k] = R2[k];
    double yaw = 0.0;
    if (fabs(R2[6]) < 1.0) { double pitch = -asin(R2[6]); double tcs = cos(pitch); yaw = atan2(R2[3] / tcs, R2[0] / tcs); }
    *yaw_out = yaw;
}

#endif
