// k_tagpose.hip — per-tag pose, AprilTag-3's estimate_tag_pose: homography -> orthogonal iteration (Lu, Hager & Mjolsness
// 2000) -> second local minimum (Schweighofer & Pinz 2006, AprilTag-3's fix_pose_ambiguities) -> the lower error first.
// DESIGN.md §Per-tag pose is the contract this file and tests/np_tag_pose.py both follow, step for step.  All arithmetic is f64.
//
// One lane per detection, 64-lane blocks (k_glue's launch shape), on the handle's stream.  A lane runs two chains of n_iters
// dependent steps, each with a 3x3 Jacobi SVD: the kernel's time is one lane's latency chain, not the detection count.  Every
// per-point array is indexed by compile-time constants (the 4-point and 3x3 loops unroll; the root finder's root lists are
// written through selects), so nothing goes to scratch.
#include <math.h>
#include <string.h>

#include "ck_internal.h"
#include "ck_mat3.h"
#define CKS_HOMOGRAPHY_ONLY
#include "ck_subpix_math.h"

namespace {

constexpr double POLY_MAX_ROOT = 1000.0; // roots are searched in [-1000, 1000] (AprilTag-3's solve_poly_approx)
constexpr double MIN_DISTINCT_BETA = 0.1; // a second minimum must differ from the first by more than this angle (rad)
constexpr double SINGULAR_G = 1e-12;     // |det G| <= this * |g1| |g2| |g3|: the corners do not span a quadrilateral

// value of the polynomial p[0] + p[1] x + ... + p[D] x^D (Horner)
template <int D>
__device__ inline double horner(const double *p, double x) {
    double v = p[D];
#pragma unroll
    for (int i = D - 1; i >= 0; i--) v = v * x + p[i];
    return v;
}
// r[n] = x for a runtime n < D, written through selects (no runtime-indexed local array)
template <int D>
__device__ inline void put_root(double *r, int n, double x) {
#pragma unroll
    for (int k = 0; k < D; k++)
        if (k == n) r[k] = x;
}
// Real roots of a degree-D polynomial in [-POLY_MAX_ROOT, POLY_MAX_ROOT], ascending: the roots of the derivative bracket the
// monotone pieces; a piece whose ends differ in sign holds one root, found by safeguarded Newton / bisection.  A vanishing
// leading coefficient needs no special case above degree 1: the derivatives inherit it, and at degree 1 a zero slope (or a
// root outside the search range) gives no root.
template <int D>
struct Poly {
    static __device__ int roots(const double *p, double *r) {
        double pd[D];
#pragma unroll
        for (int i = 0; i < D; i++) pd[i] = (double)(i + 1) * p[i + 1];
        double dr[D - 1];
#pragma unroll
        for (int i = 0; i < D - 1; i++) dr[i] = 0.0;
        const int nd = Poly<D - 1>::roots(pd, dr);
        int n = 0;
#pragma unroll
        for (int i = 0; i < D; i++) {
            if (i > nd) continue;
            const double lo = i == 0 ? -POLY_MAX_ROOT : dr[i > 0 ? i - 1 : 0];
            const double hi = i == nd ? POLY_MAX_ROOT : dr[i < D - 1 ? i : 0];
            const double flo = horner<D>(p, lo), fhi = horner<D>(p, hi);
            if (flo * fhi < 0) {
                double lower = hi, upper = lo; // p(lower) < 0 < p(upper)
                if (flo < fhi) { lower = lo; upper = hi; }
                double root = 0.5 * (lower + upper), dx_old = upper - lower, dx = dx_old;
                double f = horner<D>(p, root), df = horner<D - 1>(pd, root);
                for (int j = 0; j < 100; j++) {
                    if (f == 0.0) break;
                    if (((root - upper) * df - f) * ((root - lower) * df - f) > 0 || fabs(2.0 * f) > fabs(dx_old * df)) {
                        dx_old = dx; dx = 0.5 * (upper - lower); root = lower + dx; // bisection
                    } else {
                        dx_old = dx; dx = -f / df; root += dx;                      // Newton
                    }
                    if (root == upper || root == lower) break;
                    f = horner<D>(p, root); df = horner<D - 1>(pd, root);
                    if (f > 0) upper = root; else lower = root;
                }
                put_root<D>(r, n, root); n++;
            } else if (fhi == 0.0) {
                put_root<D>(r, n, hi); n++; // a double root at the end of the piece
            }
        }
        return n;
    }
};
template <>
struct Poly<1> {
    static __device__ int roots(const double *p, double *r) {
        if (p[1] == 0.0 || fabs(p[0]) > POLY_MAX_ROOT * fabs(p[1])) return 0;
        r[0] = -p[0] / p[1];
        return 1;
    }
};

__device__ inline bool finite9(const double m[9]) {
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 9; i++) ok = ok && isfinite(m[i]);
    return ok;
}

// The projective map of the tag square onto four points (ck_subpix_math.h: the corner refinement recomputes a detection's centre with
// the same text)
__device__ inline bool square_homography(const double x[4], const double y[4], double G[9]) { return cks_square_homography(x, y, G) != 0; }

// One orthogonal-iteration run from R (AprilTag-3's orthogonal_iteration): n_iters steps, no early exit; t of the last step
// predates its rotation update.  p: object points (p_mean is 0 exactly for the square), F: v v^T / v^T v, Minv: (I - mean F)^-1.
__device__ inline double orthogonal_iteration(const double p[4][3], const double F[4][9], const double Minv[9], int n_iters,
                                              double R[9], double t[3]) {
    double err = 0.0;
    for (int it = 0; it < n_iters; it++) {
        double Rp[4][3], acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            double fr[3];
            mat3_vec(R, p[i], Rp[i]);
            mat3_vec(F[i], Rp[i], fr);
#pragma unroll
            for (int k = 0; k < 3; k++) acc[k] += fr[k] - Rp[i][k];     // (F_i - I) R p_i
        }
#pragma unroll
        for (int k = 0; k < 3; k++) acc[k] *= 0.25;
        mat3_vec(Minv, acc, t);
        double q[4][3], qm[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const double w[3] = {Rp[i][0] + t[0], Rp[i][1] + t[1], Rp[i][2] + t[2]};
            mat3_vec(F[i], w, q[i]);
#pragma unroll
            for (int k = 0; k < 3; k++) qm[k] += q[i][k];
        }
        double pm[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int k = 0; k < 3; k++) pm[k] += p[i][k];
#pragma unroll
        for (int k = 0; k < 3; k++) { qm[k] *= 0.25; pm[k] *= 0.25; }
        double M[9];
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int b = 0; b < 3; b++) {
                double s = 0.0;
#pragma unroll
                for (int i = 0; i < 4; i++) s += (q[i][a] - qm[a]) * (p[i][b] - pm[b]);
                M[a * 3 + b] = s;
            }
        polar_rotation(M, R);
        err = 0.0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            double w[3], fw[3];
            mat3_vec(R, p[i], w);
#pragma unroll
            for (int k = 0; k < 3; k++) w[k] += t[k];
            mat3_vec(F[i], w, fw);
#pragma unroll
            for (int k = 0; k < 3; k++) { const double e = w[k] - fw[k]; err += e * e; }
        }
    }
    return err;
}

__device__ inline void calc_F(const double v[3], double F[9]) {
    const double n = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) F[a * 3 + b] = (v[a] * v[b]) / n;
}
__device__ inline bool inverse_I_minus_mean(const double F[4][9], double Minv[9]) {
    double A[9];
#pragma unroll
    for (int k = 0; k < 9; k++) A[k] = (k % 4 == 0 ? 1.0 : 0.0) - (((F[0][k] + F[1][k]) + F[2][k]) + F[3][k]) * 0.25;
    return mat3_try_inverse(A, Minv) && finite9(Minv);
}

// The second local minimum of E along the one-parameter family through (R, t) (Schweighofer & Pinz; AprilTag-3's
// fix_pose_ambiguities).  true with R2 = the seed of the second run when exactly one minimum other than the first is found.
__device__ inline bool second_minimum(const double p[4][3], const double v[4][3], const double R[9], const double t[3], double R2[9]) {
    const double tn = sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
    const double th[3] = {t[0] / tn, t[1] / tn, t[2] / tn};
    double e1[3] = {1.0 - th[0] * th[0], -th[0] * th[1], -th[0] * th[2]};
    const double e1n = sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]);
#pragma unroll
    for (int k = 0; k < 3; k++) e1[k] /= e1n;
    const double e2[3] = {th[1] * e1[2] - th[2] * e1[1], th[2] * e1[0] - th[0] * e1[2], th[0] * e1[1] - th[1] * e1[0]};
    const double Rt[9] = {e1[0], e1[1], e1[2], e2[0], e2[1], e2[2], th[0], th[1], th[2]};
    if (!finite9(Rt)) return false;
    double Rp[9];
    mat3_mul(Rt, R, Rp);
    double r31 = Rp[6], r32 = Rp[7], hyp = sqrt(r31 * r31 + r32 * r32);
    if (hyp < 1e-100) { r31 = 1.0; r32 = 0.0; hyp = 1.0; }
    const double cz = r31 / hyp, sz = r32 / hyp;
    const double Rz[9] = {cz, -sz, 0.0, sz, cz, 0.0, 0.0, 0.0, 1.0};
    double Rtr[9];
    mat3_mul(Rp, Rz, Rtr);
    const double sg = -Rtr[1], cg = Rtr[4];
    const double Rg[9] = {cg, -sg, 0.0, sg, cg, 0.0, 0.0, 0.0, 1.0};
    const double beta0 = atan2(-Rtr[6], Rtr[8]);
    // the problem in the rotated frames: p' = Rz^T p, v' = Rt v
    const double RzT[9] = {cz, sz, 0.0, -sz, cz, 0.0, 0.0, 0.0, 1.0};
    double pp[4][3], Fp[4][9];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        double vp[3];
        mat3_vec(RzT, p[i], pp[i]);
        mat3_vec(Rt, v[i], vp);
        calc_F(vp, Fp[i]);
    }
    double Gm[9];
    if (!inverse_I_minus_mean(Fp, Gm)) return false;
#pragma unroll
    for (int k = 0; k < 9; k++) Gm[k] *= 0.25;
    // Rg M_k p'_i for M_0 = I, M_1 = [[0,0,2],[0,0,0],[-2,0,0]], M_2 = diag(-1,1,-1)
    double Mp[3][4][3];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const double m1[3] = {2.0 * pp[i][2], 0.0, -2.0 * pp[i][0]}, m2[3] = {-pp[i][0], pp[i][1], -pp[i][2]};
        mat3_vec(Rg, pp[i], Mp[0][i]);
        mat3_vec(Rg, m1, Mp[1][i]);
        mat3_vec(Rg, m2, Mp[2][i]);
    }
    // (1 + tau^2) t(tau) = b_0 + tau b_1 + tau^2 b_2, b_k = Gm sum_i (F'_i - I) Rg M_k p'_i
    double bk[3][3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        double s[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            double fm[3];
            mat3_vec(Fp[i], Mp[k][i], fm);
#pragma unroll
            for (int c = 0; c < 3; c++) s[c] += fm[c] - Mp[k][i][c];
        }
        mat3_vec(Gm, s, bk[k]);
    }
    // (1 + tau^2)^2 E(tau) = a0 + a1 tau + ... + a4 tau^4 from c_k = (I - F'_i)(Rg M_k p'_i + b_k)
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        double c[3][3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double w[3] = {Mp[k][i][0] + bk[k][0], Mp[k][i][1] + bk[k][1], Mp[k][i][2] + bk[k][2]};
            double fw[3];
            mat3_vec(Fp[i], w, fw);
#pragma unroll
            for (int q = 0; q < 3; q++) c[k][q] = w[q] - fw[q];
        }
        const double c00 = c[0][0] * c[0][0] + c[0][1] * c[0][1] + c[0][2] * c[0][2];
        const double c01 = c[0][0] * c[1][0] + c[0][1] * c[1][1] + c[0][2] * c[1][2];
        const double c11 = c[1][0] * c[1][0] + c[1][1] * c[1][1] + c[1][2] * c[1][2];
        const double c02 = c[0][0] * c[2][0] + c[0][1] * c[2][1] + c[0][2] * c[2][2];
        const double c12 = c[1][0] * c[2][0] + c[1][1] * c[2][1] + c[1][2] * c[2][2];
        const double c22 = c[2][0] * c[2][0] + c[2][1] * c[2][1] + c[2][2] * c[2][2];
        a0 += c00; a1 += 2.0 * c01; a2 += c11 + 2.0 * c02; a3 += 2.0 * c12; a4 += c22;
    }
    // stationary points: roots of the numerator of dE/dtau
    const double P[5] = {a1, 2.0 * a2 - 4.0 * a0, 3.0 * a3 - 3.0 * a1, 4.0 * a4 - 2.0 * a2, -a3};
    double roots[4] = {0.0, 0.0, 0.0, 0.0};
    const int nr = Poly<4>::roots(P, roots);
    int kept = 0;
    double tau = 0.0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        if (i >= nr) continue;
        const double x = roots[i];
        const double dP = P[1] + x * (2.0 * P[2] + x * (3.0 * P[3] + x * (4.0 * P[4])));
        if (dP > 0.0 && fabs(2.0 * atan(x) - beta0) > MIN_DISTINCT_BETA) { kept++; tau = x; }
    }
    if (kept != 1) return false;
    const double den = 1.0 + tau * tau;
    const double cb = (1.0 - tau * tau) / den, sb = (2.0 * tau) / den;
    const double Rb[9] = {cb, 0.0, sb, 0.0, 1.0, 0.0, -sb, 0.0, cb};
    const double RtT[9] = {Rt[0], Rt[3], Rt[6], Rt[1], Rt[4], Rt[7], Rt[2], Rt[5], Rt[8]};
    double A[9], B[9];
    mat3_mul(RtT, Rg, A);
    mat3_mul(A, Rb, B);
    mat3_mul(B, RzT, R2);
    return finite9(R2);
}

struct TagPoseArgs {
    ck_tag_pose_params_t pp;
    ck_camera_t cam;            // pp.cam or the handle's camera (ck_kernel_camera): what the corners are undistorted with
    int n_families;
    const ck_detection_t *dets; // ck_estimate_tag_poses: [n]; ck_last_tag_poses: ws.d_dets [frames][det_cap]
    ck_tag_pose_t *out;         // [n] / [frames][cap_eff]
    int n;                      // lanes with work: records / frames * cap_eff
    const uint32_t *counters;   // ck_last_tag_poses: ws.d_counters; null for ck_estimate_tag_poses
    int det_cap, cap_eff, frames;
    int32_t *counts;            // [frames]
};

// writes one record field by field (a record assembled in a local struct would live in scratch)
__device__ inline void store_record(ck_tag_pose_t *o, int id, int family, int valid, int has_alt, const double R[9], const double t[3],
                                    double err, const double Ra[9], const double ta[3], double err_alt, const double H[9]) {
    o->id = id; o->family = family; o->valid = valid; o->has_alt = has_alt;
#pragma unroll
    for (int k = 0; k < 9; k++) { o->R[k] = R[k]; o->R_alt[k] = Ra[k]; o->H[k] = H[k]; }
#pragma unroll
    for (int k = 0; k < 3; k++) { o->t[k] = t[k]; o->t_alt[k] = ta[k]; }
    o->err = err; o->err_alt = err_alt;
}
__device__ inline void store_invalid(ck_tag_pose_t *o, int id, int family) {
    const double z[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    store_record(o, id, family, 0, 0, z, z, 0.0, z, z, 0.0, z);
}

__device__ void tag_pose(const ck_detection_t &d, const ck_tag_pose_params_t &pp, const ck_camera_t &cam, int n_families, ck_tag_pose_t *o) {
    const int fam = d.family;
    if (fam < 0 || fam >= n_families) { store_invalid(o, d.id, d.family); return; }
    const double tagsize = fam == 0 ? pp.tagsize[0] : (fam == 1 ? pp.tagsize[1] : (fam == 2 ? pp.tagsize[2] : pp.tagsize[3]));
    const double s = 0.5 * tagsize;
    double u[4], w[4], x[4] = {0, 0, 0, 0}, y[4] = {0, 0, 0, 0};
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        u[i] = d.p[i][0]; w[i] = d.p[i][1];
        ok = ok && isfinite(u[i]) && isfinite(w[i]);
    }
#pragma unroll
    for (int i = 0; i < 4; i++) ok = ok && camera_undistort_one(cam, u[i], w[i], &x[i], &y[i]);
    // initial pose from the homography of the normalised points
    double G[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    ok = ok && square_homography(x, y, G) && square_homography(u, w, H);
    const double n1 = sqrt(G[0] * G[0] + G[3] * G[3] + G[6] * G[6]), n2 = sqrt(G[1] * G[1] + G[4] * G[4] + G[7] * G[7]);
    const double n3 = sqrt(G[2] * G[2] + G[5] * G[5] + G[8] * G[8]);
    ok = ok && fabs(mat3_det(G)) > SINGULAR_G * (n1 * n2 * n3);
    const double h8 = H[8];
#pragma unroll
    for (int k = 0; k < 9; k++) H[k] /= h8;
    ok = ok && finite9(H);
    double lam = 1.0 / sqrt(n1 * n2);
    if (G[8] < 0.0) lam = -lam;
    const double r1[3] = {lam * G[0], lam * G[3], lam * G[6]}, r2[3] = {lam * G[1], lam * G[4], lam * G[7]};
    const double r3[3] = {r1[1] * r2[2] - r1[2] * r2[1], r1[2] * r2[0] - r1[0] * r2[2], r1[0] * r2[1] - r1[1] * r2[0]};
    const double M0[9] = {r1[0], r2[0], r3[0], r1[1], r2[1], r3[1], r1[2], r2[2], r3[2]};
    double R[9], t[3] = {s * lam * G[2], s * lam * G[5], s * lam * G[8]};
    ok = ok && finite9(M0) && isfinite(t[0]) && isfinite(t[1]) && isfinite(t[2]);
    if (!ok) { store_invalid(o, d.id, d.family); return; }
    polar_rotation(M0, R);
    // orthogonal iteration from the homography's rotation
    const double p[4][3] = {{-s, s, 0.0}, {s, s, 0.0}, {s, -s, 0.0}, {-s, -s, 0.0}};
    double v[4][3], F[4][9], Minv[9];
#pragma unroll
    for (int i = 0; i < 4; i++) { v[i][0] = x[i]; v[i][1] = y[i]; v[i][2] = 1.0; calc_F(v[i], F[i]); }
    ok = finite9(R) && inverse_I_minus_mean(F, Minv);
    if (!ok) { store_invalid(o, d.id, d.family); return; }
    double err = orthogonal_iteration(p, F, Minv, pp.n_iters, R, t);
    if (!finite9(R) || !isfinite(t[0]) || !isfinite(t[1]) || !isfinite(t[2]) || !isfinite(err)) { store_invalid(o, d.id, d.family); return; }
    // the second minimum, refined by its own run
    double R2[9], t2[3] = {0.0, 0.0, 0.0}, err2 = INFINITY;
    bool alt = second_minimum(p, v, R, t, R2);
    if (alt) {
        err2 = orthogonal_iteration(p, F, Minv, pp.n_iters, R2, t2);
        alt = finite9(R2) && isfinite(t2[0]) && isfinite(t2[1]) && isfinite(t2[2]) && isfinite(err2);
    }
    const bool swap = alt && err2 < err; // the lower error first; on a tie the homography-seeded solution
    double Ro[9], to[3], Ra[9], ta[3];
#pragma unroll
    for (int k = 0; k < 9; k++) { Ro[k] = swap ? R2[k] : R[k]; Ra[k] = alt ? (swap ? R[k] : R2[k]) : 0.0; }
#pragma unroll
    for (int k = 0; k < 3; k++) { to[k] = swap ? t2[k] : t[k]; ta[k] = alt ? (swap ? t[k] : t2[k]) : 0.0; }
    store_record(o, d.id, d.family, 1, alt ? 1 : 0, Ro, to, swap ? err2 : err, Ra, ta, alt ? (swap ? err : err2) : INFINITY, H);
}

constexpr int TP_NT = 64;
__global__ __launch_bounds__(TP_NT) void k_tagpose(TagPoseArgs a) {
    const int i = blockIdx.x * TP_NT + threadIdx.x;
    if (a.counters && i < a.frames) { // ck_last_tag_poses: the per-frame counts
        uint32_t nd = a.counters[(size_t)i * CK_CNT_STRIDE + CK_CNT_DETS];
        if (nd > (uint32_t)a.cap_eff) nd = (uint32_t)a.cap_eff;
        a.counts[i] = (int32_t)nd;
    }
    if (i >= a.n) return;
    if (a.counters) {
        const int f = i / a.cap_eff, k = i - f * a.cap_eff;
        uint32_t nd = a.counters[(size_t)f * CK_CNT_STRIDE + CK_CNT_DETS];
        if (nd > (uint32_t)a.cap_eff) nd = (uint32_t)a.cap_eff;
        if ((uint32_t)k >= nd) { store_invalid(&a.out[i], 0, 0); return; } // past the frame's detections: a zero record
        const ck_detection_t d = a.dets[(size_t)f * a.det_cap + k];
        tag_pose(d, a.pp, a.cam, a.n_families, &a.out[i]);
    } else {
        const ck_detection_t d = a.dets[i];
        tag_pose(d, a.pp, a.cam, a.n_families, &a.out[i]);
    }
}

int check_params(const ck_handle *h, const ck_tag_pose_params_t *pp) {
    const ck_opencv5_t &c = pp->cam;
    if (!h->has_camera) { // (a camera set on the handle was checked by ck_set_camera; the params' field is ignored then)
        if (!isfinite(c.fx) || !isfinite(c.fy) || !(c.fx > 0.0) || !(c.fy > 0.0)) return CK_EINVAL;
        const double rest[7] = {c.cx, c.cy, c.k1, c.k2, c.p1, c.p2, c.k3};
        for (double v : rest)
            if (!isfinite(v)) return CK_EINVAL;
    }
    for (int i = 0; i < h->cfg.n_families; i++)
        if (!isfinite(pp->tagsize[i]) || !(pp->tagsize[i] > 0.0)) return CK_EINVAL;
    if (pp->n_iters < 1 || pp->n_iters > 1000) return CK_EINVAL;
    return CK_OK;
}

// the pose buffers, allocated by the first call that needs them (ck_create allocates exactly what it did before)
int alloc_buffers(ck_handle *h) {
    int rc = ck_buf_alloc(h, &h->d_tp_dets);
    if (rc == CK_OK) rc = ck_buf_alloc(h, &h->d_tp_counts);
    if (rc == CK_OK) rc = ck_buf_alloc(h, &h->d_tp_out);
    return rc; // (what a failure leaves allocated is kept for the next call, and released with the handle)
}

TagPoseArgs make_args(const ck_handle *h, const ck_tag_pose_params_t *pp) {
    TagPoseArgs a;
    memset(&a, 0, sizeof a);
    a.pp = *pp; a.cam = ck_kernel_camera(h, pp->cam); a.n_families = h->cfg.n_families; a.out = h->d_tp_out; a.det_cap = h->ws.det_cap;
    return a;
}

} // namespace

static_assert(sizeof(ck_tag_pose_params_t) == 112, "ck_tag_pose_params_t layout");
static_assert(sizeof(ck_tag_pose_t) == 296, "ck_tag_pose_t layout");

extern "C" void ck_tag_pose_params_default(ck_tag_pose_params_t *pp) {
    if (!pp) return;
    memset(pp, 0, sizeof *pp);
    for (int i = 0; i < CK_MAX_FAMILIES; i++) pp->tagsize[i] = TAG_SIZE;
    pp->n_iters = 50;                                                   // estimate_tag_pose's orthogonal-iteration steps
}

extern "C" int ck_estimate_tag_poses(ck_handle_t *h, const ck_tag_pose_params_t *pp, const ck_detection_t *dets, int32_t n,
                                     ck_tag_pose_t *out) {
    if (!h || !pp || !dets || !out || n < 0) return CK_EINVAL;
    int rc = check_params(h, pp);
    if (rc != CK_OK) return rc;
    if ((int64_t)n > (int64_t)h->cfg.max_batch * h->ws.det_cap) return CK_ECAPACITY;
    if (n == 0) return CK_OK;
    CK_HIP(hipSetDevice(h->device));
    rc = alloc_buffers(h);
    if (rc != CK_OK) return rc;
    CK_HIP(hipMemcpyAsync(h->d_tp_dets, dets, sizeof(ck_detection_t) * (size_t)n, hipMemcpyDefault, h->stream));
    TagPoseArgs a = make_args(h, pp);
    a.dets = h->d_tp_dets; a.n = n;
    hipLaunchKernelGGL(k_tagpose, dim3((unsigned)((n + TP_NT - 1) / TP_NT)), dim3(TP_NT), 0, h->stream, a);
    CK_HIP(hipGetLastError());
    CK_HIP(hipMemcpyAsync(out, h->d_tp_out, sizeof(ck_tag_pose_t) * (size_t)n, hipMemcpyDefault, h->stream));
    CK_HIP(hipStreamSynchronize(h->stream));
    return CK_OK;
}

extern "C" int ck_last_tag_poses(ck_handle_t *h, const ck_tag_pose_params_t *pp, ck_tag_pose_t *out, int32_t cap_per_frame,
                                 int32_t *counts) {
    if (!h || !pp || !out || !counts || cap_per_frame < 1) return CK_EINVAL;
    int rc = check_params(h, pp);
    if (rc != CK_OK) return rc;
    if (h->n_last_dets < 1) return CK_EINVAL; // nothing detected since ck_create, or the workspace was rewritten since
    const int frames = h->n_last_dets, cap_eff = cap_per_frame < h->ws.det_cap ? cap_per_frame : h->ws.det_cap;
    CK_HIP(hipSetDevice(h->device));
    rc = alloc_buffers(h);
    if (rc != CK_OK) return rc;
    TagPoseArgs a = make_args(h, pp);
    a.dets = h->ws.d_dets; a.counters = h->ws.d_counters; a.n = frames * cap_eff; a.cap_eff = cap_eff; a.frames = frames;
    a.counts = h->d_tp_counts;
    hipLaunchKernelGGL(k_tagpose, dim3((unsigned)((a.n + TP_NT - 1) / TP_NT)), dim3(TP_NT), 0, h->stream, a);
    CK_HIP(hipGetLastError());
    const size_t rec = sizeof(ck_tag_pose_t);
    if (cap_eff == cap_per_frame)
        CK_HIP(hipMemcpyAsync(out, h->d_tp_out, rec * (size_t)frames * cap_eff, hipMemcpyDefault, h->stream));
    else // a frame holds at most det_cap detections: the records past them in `out` are not written
        CK_HIP(hipMemcpy2DAsync(out, rec * (size_t)cap_per_frame, h->d_tp_out, rec * cap_eff, rec * cap_eff, (size_t)frames,
                                hipMemcpyDefault, h->stream));
    CK_HIP(hipMemcpyAsync(counts, h->d_tp_counts, sizeof(int32_t) * (size_t)frames, hipMemcpyDefault, h->stream));
    CK_HIP(hipStreamSynchronize(h->stream));
    return CK_OK;
}
