// rigcal_host_check — the host half of the mount calibration (ck_rigcal_host.c: ck_rigcal_check, ck_rigcal_jacobian,
// ck_rigcal_refine_host) under AddressSanitizer and UBSan, driven from tests/test_cpp_rigcal.py.  Stand-alone: it links the one C file,
// not the library, and needs no device.  Makes random captures of 2 and 3 cameras (exact bearings, a camera without tags at some steps,
// one-camera steps), solves them from perturbed mounts and poses against their truth, solves a subset at offsets inside larger arrays,
// with frozen parts and three iterations, walks the refusals in their order, and prints OK.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "chalkydri_hip.h"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
double uni(double lo, double hi) { // xorshift64*
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return lo + (hi - lo) * (double)((rng_state * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0;
}

struct Mat { double m[9]; };
Mat quat_mat(const double *q) {
    const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]), w = q[0] / n, x = q[1] / n, y = q[2] / n, z = q[3] / n;
    return Mat{{1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)}};
}
void rand_quat(double amount, double *q) { // a rotation by up to `amount` radians about a random axis; amount >= 4: any rotation
    double a[3] = {uni(-1, 1), uni(-1, 1), uni(-1, 1)};
    const double n = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]), ang = amount >= 4 ? uni(-3.14, 3.14) : uni(-amount, amount);
    q[0] = std::cos(ang / 2);
    for (int i = 0; i < 3; i++) q[1 + i] = std::sin(ang / 2) * a[i] / n;
}
void quat_mul(const double *a, const double *b, double *c) {
    c[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
    c[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
    c[2] = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
    c[3] = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
}

int fail(const char *what, int v) {
    std::printf("FAIL %s %d\n", what, v);
    return 1;
}

struct Capture {
    int C, n;
    std::vector<ck_sqpnp_problem_t> rec;
    std::vector<ck_iso3_t> tags, mounts, start;
    std::vector<double> bear, poses, poses0;
};

// cameras anywhere on the robot, robot anywhere; tags(s, c) tags 1..5 m in front of camera c
Capture make(int C, int n, int (*tags)(int, int)) {
    static const double cd = 0.1651 / 2, cp[4][3] = {{0, -cd, -cd}, {0, cd, -cd}, {0, cd, cd}, {0, -cd, cd}};
    Capture K;
    K.C = C; K.n = n;
    K.rec.resize((size_t)C * n);
    K.mounts.resize(C); K.start.resize(C);
    K.poses.resize(12 * (size_t)n); K.poses0.resize(12 * (size_t)n);
    std::vector<Mat> A(C);
    std::vector<double> o(3 * C);
    for (int c = 0; c < C; c++) {
        rand_quat(4, K.mounts[c].q);
        A[c] = quat_mat(K.mounts[c].q);
        for (int i = 0; i < 3; i++) o[3 * c + i] = uni(-0.4, 0.4);
        for (int i = 0; i < 3; i++) K.mounts[c].t[i] = -(A[c].m[3 * i] * o[3 * c] + A[c].m[3 * i + 1] * o[3 * c + 1] + A[c].m[3 * i + 2] * o[3 * c + 2]);
        K.start[c] = K.mounts[c];
        if (c > 0) { // up to 2 degrees and 2 cm off: A C(dw), o + do
            double dq[4], q2[4], o2[3];
            rand_quat(0.035, dq);
            quat_mul(K.mounts[c].q, dq, q2);
            std::memcpy(K.start[c].q, q2, sizeof q2);
            const Mat A2 = quat_mat(q2);
            for (int i = 0; i < 3; i++) o2[i] = o[3 * c + i] + uni(-0.02, 0.02);
            for (int i = 0; i < 3; i++) K.start[c].t[i] = -(A2.m[3 * i] * o2[0] + A2.m[3 * i + 1] * o2[1] + A2.m[3 * i + 2] * o2[2]);
        }
    }
    for (int s = 0; s < n; s++) {
        double q[4], q0[4], dq[4];
        rand_quat(4, q);
        const Mat R = quat_mat(q);
        double t[3] = {uni(-8, 8), uni(-8, 8), uni(-0.5, 0.5)};
        std::memcpy(&K.poses[12 * s], R.m, sizeof R.m);
        std::memcpy(&K.poses[12 * s + 9], t, sizeof t);
        rand_quat(0.02, dq);
        quat_mul(q, dq, q0);
        const Mat R0 = quat_mat(q0);
        std::memcpy(&K.poses0[12 * s], R0.m, sizeof R0.m);
        for (int i = 0; i < 3; i++) K.poses0[12 * s + 9 + i] = t[i] + uni(-0.03, 0.03);
        for (int c = 0; c < C; c++) {
            ck_sqpnp_problem_t &r = K.rec[(size_t)c * n + s];
            std::memset(&r, 0, sizeof r);
            r.n_tags = tags(s, c); r.n_bearings = 4 * r.n_tags;
            r.tag_offset = (int32_t)K.tags.size(); r.bearing_offset = (int32_t)(K.bear.size() / 3);
            r.robot_to_cam.q[0] = 1;
            for (int k = 0; k < r.n_tags; k++) {
                // the tag in the camera frame, then to the world: X = R^T (A^T p_cam + o - t)
                const double z = uni(1, 5), pc[3] = {uni(-0.4, 0.4) * z, uni(-0.3, 0.3) * z, z};
                double qt[4];
                rand_quat(4, qt);
                ck_iso3_t tag;
                std::memcpy(tag.q, qt, sizeof qt);
                double pr[3];
                for (int i = 0; i < 3; i++) pr[i] = A[c].m[i] * pc[0] + A[c].m[3 + i] * pc[1] + A[c].m[6 + i] * pc[2] + o[3 * c + i] - t[i];
                for (int i = 0; i < 3; i++) tag.t[i] = R.m[i] * pr[0] + R.m[3 + i] * pr[1] + R.m[6 + i] * pr[2];
                K.tags.push_back(tag);
                const Mat Rt = quat_mat(qt);
                for (int j = 0; j < 4; j++) {
                    double X[3], w[3], p[3];
                    for (int i = 0; i < 3; i++) X[i] = Rt.m[3 * i] * cp[j][0] + Rt.m[3 * i + 1] * cp[j][1] + Rt.m[3 * i + 2] * cp[j][2] + tag.t[i];
                    for (int i = 0; i < 3; i++) w[i] = R.m[3 * i] * X[0] + R.m[3 * i + 1] * X[1] + R.m[3 * i + 2] * X[2] + t[i] - o[3 * c + i];
                    for (int i = 0; i < 3; i++) p[i] = A[c].m[3 * i] * w[0] + A[c].m[3 * i + 1] * w[1] + A[c].m[3 * i + 2] * w[2];
                    const double nn = std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
                    for (int i = 0; i < 3; i++) K.bear.push_back(p[i] / nn);
                }
            }
        }
    }
    return K;
}

double quat_angle(const double *a, const double *b) { // of conj(a) b, from its vector part: resolves angles far below 1e-8
    const double ca[4] = {a[0], -a[1], -a[2], -a[3]};
    double r[4];
    quat_mul(ca, b, r);
    return 2 * std::atan2(std::sqrt(r[1] * r[1] + r[2] * r[2] + r[3] * r[3]), std::fabs(r[0]));
}

int refine(const ck_rigcal_params_t &p, const Capture &K, const ck_rigcal_problem_t &q, const std::vector<int32_t> &idx, ck_rigcal_result_t *res,
           std::vector<double> &out) {
    return ck_rigcal_refine_host(&p, K.C, K.rec.data(), K.n, K.tags.data(), (int32_t)K.tags.size(), K.bear.data(), (int32_t)(K.bear.size() / 3), &q,
                                 idx.data(), (int32_t)idx.size(), K.start.data(), K.poses0.data(), res, out.data());
}
int check(const ck_rigcal_params_t *p, const Capture &K, int C, const ck_rigcal_problem_t *q, const std::vector<int32_t> &idx, int n_tags, int n_bear,
          const ck_iso3_t *mounts) {
    return ck_rigcal_check(p, C, K.rec.data(), K.n, K.tags.data(), n_tags, K.bear.data(), n_bear, q, 1, idx.data(), (int32_t)idx.size(), mounts);
}

int tags2(int s, int c) { return c == 1 && (s == 3 || s == 4) ? 0 : 1 + (s + c) % 3; }             // steps 3, 4: one camera, skipped
int tags3(int s, int c) { return c == 2 && s % 2 ? 0 : (s == 5 ? 5 : 2); }                       // camera 2 absent from odd steps; a 20-point view

} // namespace

int main() {
    ck_rigcal_params_t p;
    ck_rigcal_params_default(&p);
    if (p.max_iters != 100 || p.min_steps != 3 || p.min_cams_per_step != 2 || p.fixed_mask != 0) return fail("defaults", 0);
    p.fixed_mask = CK_RIGCAL_FIX_CAMERA(0);
    int iters = 0;
    for (int round = 0; round < 2; round++) {
        const Capture K = round ? make(3, 14, tags3) : make(2, 12, tags2);
        std::vector<int32_t> idx(K.n);
        for (int s = 0; s < K.n; s++) idx[s] = s;
        const ck_rigcal_problem_t q{K.n, 0};
        ck_rigcal_result_t res;
        std::vector<double> out(12 * (size_t)K.n);
        int rc = refine(p, K, q, idx, &res, out);
        if (rc != CK_OK || (res.status != CK_CALIB_CONVERGED && res.status != CK_CALIB_STALLED)) return fail("refine", rc ? rc : res.status);
        if (res.n_steps != K.n || res.n_steps_used != (round ? K.n : K.n - 2) || !(res.rms < 1e-9) || !(res.cost <= res.cost0)) return fail("record", res.n_steps_used);
        for (int c = 0; c < K.C; c++) {
            if (!(quat_angle(res.robot_to_cam[c].q, K.mounts[c].q) < 1e-7)) return fail("mount rotation", c);
            for (int i = 0; i < 3; i++)
                if (!(std::fabs(res.robot_to_cam[c].t[i] - K.mounts[c].t[i]) < 1e-7)) return fail("mount translation", c);
        }
        if (std::memcmp(&res.robot_to_cam[0], &K.start[0], sizeof(ck_iso3_t)) != 0) return fail("gauge camera", 0);
        for (int s = 0; s < K.n; s++) {
            const bool skipped = !round && (s == 3 || s == 4);
            for (int i = 0; i < 12; i++)
                if (skipped ? out[12 * s + i] != K.poses0[12 * s + i] : !(std::fabs(out[12 * s + i] - K.poses[12 * s + i]) < 1e-6)) return fail("pose", s);
        }
        iters = res.iters;
        // a subset at an offset inside a larger index array, the poses at that offset of a larger output; position of camera 1 frozen,
        // three iterations: MAXIT, and camera 1 stays where it was
        std::vector<int32_t> idx2{7, 7, 0, 2, 5, 6, 8, 9, 11, 3};
        const ck_rigcal_problem_t q2{7, 2};
        ck_rigcal_params_t p2 = p;
        p2.fixed_mask |= CK_RIGCAL_FIX_POSITION(1); p2.max_iters = 3;
        std::vector<double> out2(12 * idx2.size(), -1.0);
        rc = refine(p2, K, q2, idx2, &res, out2);
        if (rc != CK_OK || res.status != CK_CALIB_MAXIT || res.iters != 3 || res.n_steps != 7) return fail("maxit", rc ? rc : res.status);
        if (out2[0] != -1.0 || out2[12 * 2 - 1] != -1.0 || out2[12 * 9] != -1.0) return fail("poses outside the problem", 0);
        {
            const Mat A0 = quat_mat(K.start[1].q), A1 = quat_mat(res.robot_to_cam[1].q);
            for (int i = 0; i < 3; i++) { // o = -A^T b
                const double o0 = -(A0.m[i] * K.start[1].t[0] + A0.m[3 + i] * K.start[1].t[1] + A0.m[6 + i] * K.start[1].t[2]);
                const double o1 = -(A1.m[i] * res.robot_to_cam[1].t[0] + A1.m[3 + i] * res.robot_to_cam[1].t[1] + A1.m[6 + i] * res.robot_to_cam[1].t[2]);
                if (!(std::fabs(o0 - o1) < 1e-14)) return fail("frozen position", i);
            }
        }
        // the Jacobian of one point
        double r[3], J[36];
        const double X[3] = {1, 2, 0.5}, v[3] = {0.1, -0.2, 0.97}, P[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0.5, 0.25, 2};
        if (ck_rigcal_jacobian(&K.mounts[1], P, X, v, 1, 0x7, r, J) != CK_OK || J[0] != 0 || J[1] != 0 || J[2] != 0 || J[12 + 2] != 0 || J[3] == 0) return fail("jacobian", 0);
        // the refusals, in their order: the earlier wins when two apply
        const int nt = (int)K.tags.size(), nb = (int)(K.bear.size() / 3);
        ck_rigcal_params_t bad = p;
        if (check(nullptr, K, K.C, &q, idx, nt, nb, K.start.data()) != CK_EINVAL) return fail("null", 0);
        if (check(&p, K, 0, &q, idx, nt, nb, K.start.data()) != CK_EINVAL || check(&p, K, 9, &q, idx, nt, nb, K.start.data()) != CK_EINVAL) return fail("n_cams", 0);
        if (check(&p, K, K.C, &q, idx, nt - 1, nb, K.start.data()) != CK_EINVAL) return fail("tags outside", 0);
        if (check(&p, K, K.C, &q, idx, nt, nb - 1, K.start.data()) != CK_EINVAL) return fail("bearings outside", 0);
        {
            Capture B = K;
            B.rec[1].n_bearings -= 1;
            if (check(&p, B, B.C, &q, idx, nt, nb, B.start.data()) != CK_EINVAL) return fail("4 n_tags", 0);
        }
        {
            std::vector<int32_t> i3 = idx;
            i3[4] = i3[3];
            if (check(&p, K, K.C, &q, i3, nt, nb, K.start.data()) != CK_EINVAL) return fail("not increasing", 0);
            i3[4] = K.n;
            if (check(&p, K, K.C, &q, i3, nt, nb, K.start.data()) != CK_EINVAL) return fail("step out of range", 0);
            const ck_rigcal_problem_t past{K.n, 1};
            if (check(&p, K, K.C, &past, idx, nt, nb, K.start.data()) != CK_EINVAL) return fail("index outside", 0);
        }
        bad.max_iters = 0;
        if (check(&bad, K, K.C, &q, idx, nt, nb, K.start.data()) != CK_EINVAL) return fail("max_iters", 0);
        bad = p; bad.max_iters = 10001;
        if (check(&bad, K, K.C, &q, idx, nt, nb, K.start.data()) != CK_EINVAL) return fail("max_iters high", 0);
        bad = p; bad.min_steps = 0;
        if (check(&bad, K, K.C, &q, idx, nt, nb, K.start.data()) != CK_EINVAL) return fail("min_steps", 0);
        bad = p; bad.min_cams_per_step = 1;
        if (check(&bad, K, K.C, &q, idx, nt, nb, K.start.data()) != CK_EINVAL) return fail("min_cams_per_step", 0);
        {
            Capture B = K;
            B.bear[5] = NAN;
            if (check(&p, B, B.C, &q, idx, nt, nb, B.start.data()) != CK_EINVAL) return fail("not finite", 0);
            B = K;
            B.start[1].t[2] = INFINITY;
            if (check(&p, B, B.C, &q, idx, nt, nb, B.start.data()) != CK_EINVAL) return fail("mount not finite", 0);
        }
        bad = p; bad.fixed_mask = CK_RIGCAL_FIX_POSITION(0) | CK_RIGCAL_FIX_POSITION(1);
        if (check(&bad, K, K.C, &q, idx, nt, nb, K.start.data()) != CK_EINVAL) return fail("gauge", 0);
        {
            std::vector<int32_t> big(CK_RIGCAL_MAX_STEPS + 1, 0);
            const ck_rigcal_problem_t qb{CK_RIGCAL_MAX_STEPS + 1, 0};
            if (check(&p, K, K.C, &qb, big, nt, nb, K.start.data()) != CK_EINVAL) return fail("capacity after order", 0); // (not increasing comes first)
        }
        if (check(&p, K, K.C, &q, idx, nt, nb, K.start.data()) != CK_OK) return fail("valid", 0);
    }
    // beyond CK_RIGCAL_MAX_STEPS: a capture of that many empty steps plus one with tags
    {
        Capture K = make(2, 3, tags2);
        const int n = CK_RIGCAL_MAX_STEPS + 1;
        std::vector<ck_sqpnp_problem_t> rec((size_t)2 * n);
        std::memset(rec.data(), 0, sizeof(ck_sqpnp_problem_t) * rec.size());
        rec[0] = K.rec[0]; rec[n] = K.rec[3];
        std::vector<int32_t> idx(n);
        for (int s = 0; s < n; s++) idx[s] = s;
        const ck_rigcal_problem_t q{n, 0};
        const int rc = ck_rigcal_check(&p, 2, rec.data(), n, K.tags.data(), (int32_t)K.tags.size(), K.bear.data(), (int32_t)(K.bear.size() / 3), &q, 1,
                                       idx.data(), n, K.start.data());
        if (rc != CK_ECAPACITY) return fail("capacity", rc);
    }
    std::printf("OK %d iterations\n", iters);
    return 0;
}
