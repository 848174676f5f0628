// fieldcal_host_check — the host half of the field calibration (ck_fieldcal_host.c: ck_fieldcal_check, ck_fieldcal_jacobian,
// ck_fieldcal_refine_host) under AddressSanitizer and UBSan, driven from tests/test_cpp_fieldcal.py.  Stand-alone: it links the two C
// files it needs, not the library, and needs no device.  Makes random captures of 1 and 3 cameras over a layout of 9 tags (exact
// bearings, one-tag steps, a tag seen by several cameras at once, a layout entry never seen), solves them from a perturbed layout and
// perturbed poses against their truth, solves a subset at offsets inside larger arrays with frozen parts and three iterations, walks
// the refusals in their order, and prints OK.
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
double quat_angle(const double *a, const double *b) { // of conj(a) b, from its vector part: resolves angles far below 1e-8
    const double ca[4] = {a[0], -a[1], -a[2], -a[3]};
    double r[4];
    quat_mul(ca, b, r);
    return 2 * std::atan2(std::sqrt(r[1] * r[1] + r[2] * r[2] + r[3] * r[3]), std::fabs(r[0]));
}

int fail(const char *what, int v) {
    std::printf("FAIL %s %d\n", what, v);
    return 1;
}

constexpr int L = 9; // layout entries; the last is never seen

struct Capture {
    int C, n;
    std::vector<ck_sqpnp_problem_t> rec;
    std::vector<int32_t> tag_index;
    std::vector<ck_iso3_t> mounts, truth, layout0;
    std::vector<uint8_t> fixed;
    std::vector<double> bear, poses, poses0;
};

// cameras anywhere on the robot, the robot within 3 m of the origin, tags on a ring of 6 m; camera c at step s sees the tags
// first(s, c) .. first(s, c) + count(s, c) - 1 (mod L - 1) wherever they are: a bearing is any direction
Capture make(int C, int n, int (*first)(int, int), int (*count)(int, int)) {
    static const double cd = 0.1651 / 2, cp[4][3] = {{0, -cd, -cd}, {0, cd, -cd}, {0, cd, cd}, {0, -cd, cd}};
    Capture K;
    K.C = C; K.n = n;
    K.rec.resize((size_t)C * n);
    K.mounts.resize(C); K.truth.resize(L); K.layout0.resize(L); K.fixed.assign(L, 0);
    K.poses.resize(12 * (size_t)n); K.poses0.resize(12 * (size_t)n);
    std::vector<Mat> A(C);
    std::vector<double> o(3 * C);
    for (int c = 0; c < C; c++) {
        rand_quat(4, K.mounts[c].q);
        A[c] = quat_mat(K.mounts[c].q);
        for (int i = 0; i < 3; i++) o[3 * c + i] = uni(-0.4, 0.4);
        for (int i = 0; i < 3; i++) K.mounts[c].t[i] = -(A[c].m[3 * i] * o[3 * c] + A[c].m[3 * i + 1] * o[3 * c + 1] + A[c].m[3 * i + 2] * o[3 * c + 2]);
    }
    for (int k = 0; k < L; k++) {
        const double a = 6.28318 * k / L;
        rand_quat(4, K.truth[k].q);
        K.truth[k].t[0] = 6 * std::cos(a); K.truth[k].t[1] = 6 * std::sin(a); K.truth[k].t[2] = uni(0.3, 1.5);
        K.layout0[k] = K.truth[k];
        if (k > 0) { // up to 2 degrees and 2 cm off
            double dq[4];
            rand_quat(0.035, dq);
            quat_mul(K.truth[k].q, dq, K.layout0[k].q);
            for (int i = 0; i < 3; i++) K.layout0[k].t[i] += uni(-0.02, 0.02);
        }
    }
    K.fixed[0] = CK_FIELDCAL_FIX_ALL;
    for (int s = 0; s < n; s++) {
        double q[4], q0[4], dq[4];
        rand_quat(4, q);
        const Mat R = quat_mat(q);
        double t[3] = {uni(-3, 3), uni(-3, 3), uni(-0.5, 0.5)};
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
            r.n_tags = count(s, c); r.n_bearings = 4 * r.n_tags;
            r.tag_offset = (int32_t)K.tag_index.size(); r.bearing_offset = (int32_t)(K.bear.size() / 3);
            r.robot_to_cam.q[0] = 1;
            for (int k = 0; k < r.n_tags; k++) {
                const int id = (first(s, c) + k) % (L - 1);
                K.tag_index.push_back(id);
                const Mat Rt = quat_mat(K.truth[id].q);
                for (int j = 0; j < 4; j++) {
                    double X[3], w[3], p[3];
                    for (int i = 0; i < 3; i++) X[i] = Rt.m[3 * i] * cp[j][0] + Rt.m[3 * i + 1] * cp[j][1] + Rt.m[3 * i + 2] * cp[j][2] + K.truth[id].t[i];
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

struct Out {
    ck_fieldcal_result_t res;
    std::vector<ck_iso3_t> layout;
    std::vector<int32_t> sight;
    std::vector<double> rms, poses;
};

int refine(const ck_fieldcal_params_t &p, const Capture &K, const ck_rigcal_problem_t &q, const std::vector<int32_t> &idx, Out &o) {
    o.layout.resize(L); o.sight.assign(L, -1); o.rms.assign(L, -1.0);
    return ck_fieldcal_refine_host(&p, K.C, K.rec.data(), K.n, K.tag_index.data(), (int32_t)K.tag_index.size(), K.bear.data(),
                                   (int32_t)(K.bear.size() / 3), &q, idx.data(), (int32_t)idx.size(), K.mounts.data(), K.layout0.data(), L,
                                   K.fixed.data(), K.poses0.data(), &o.res, o.layout.data(), o.sight.data(), o.rms.data(), o.poses.data());
}
int check(const ck_fieldcal_params_t *p, const Capture &K, int C, const ck_rigcal_problem_t *q, const std::vector<int32_t> &idx, int n_tags, int n_bear,
          int n_layout = L) {
    return ck_fieldcal_check(p, C, K.rec.data(), K.n, K.tag_index.data(), n_tags, K.bear.data(), n_bear, q, 1, idx.data(), (int32_t)idx.size(),
                             K.mounts.data(), K.layout0.data(), n_layout, K.fixed.data());
}

int first1(int s, int) { return 3 * s; }
int count1(int s, int) { return s == 3 || s == 4 ? 1 : 2 + s % 3; }                                // steps 3, 4: one tag, skipped
int first3(int s, int c) { return s + (c == 2 ? 1 : 0); }                                         // cameras 0 and 1 see the same tags
int count3(int s, int c) { return c == 2 && s % 2 ? 0 : (s == 5 ? 5 : 2); }                       // camera 2 absent from odd steps

} // namespace

int main() {
    ck_fieldcal_params_t p;
    ck_fieldcal_params_default(&p);
    if (p.max_iters != 100 || p.min_steps != 3 || p.min_tags_per_step != 2) return fail("defaults", 0);
    int iters = 0;
    for (int round = 0; round < 2; round++) {
        const Capture K = round ? make(3, 16, first3, count3) : make(1, 14, first1, count1);
        std::vector<int32_t> idx(K.n);
        for (int s = 0; s < K.n; s++) idx[s] = s;
        const ck_rigcal_problem_t q{K.n, 0};
        Out o;
        o.poses.assign(12 * (size_t)K.n, 0.0);
        int rc = refine(p, K, q, idx, o);
        if (rc != CK_OK || (o.res.status != CK_CALIB_CONVERGED && o.res.status != CK_CALIB_STALLED)) return fail("refine", rc ? rc : o.res.status);
        if (o.res.n_steps != K.n || o.res.n_steps_used != (round ? K.n : K.n - 2) || !(o.res.rms < 1e-9) || !(o.res.cost <= o.res.cost0)) return fail("record", o.res.n_steps_used);
        if (o.res.n_tags_solved != L - 2 || o.res.n_points != 4 * (o.sight[0] + o.sight[1] + o.sight[2] + o.sight[3] + o.sight[4] + o.sight[5] + o.sight[6] + o.sight[7]))
            return fail("counts", o.res.n_tags_solved);
        for (int k = 0; k < L - 1; k++) {
            if (o.sight[k] < 1 || !(o.rms[k] < 1e-9)) return fail("tag record", k);
            if (!(quat_angle(o.layout[k].q, K.truth[k].q) < 1e-7)) return fail("tag rotation", k);
            for (int i = 0; i < 3; i++)
                if (!(std::fabs(o.layout[k].t[i] - K.truth[k].t[i]) < 1e-7)) return fail("tag translation", k);
        }
        if (std::memcmp(&o.layout[0], &K.layout0[0], sizeof(ck_iso3_t)) != 0) return fail("gauge tag", 0);
        if (std::memcmp(&o.layout[L - 1], &K.layout0[L - 1], sizeof(ck_iso3_t)) != 0 || o.sight[L - 1] != 0 || o.rms[L - 1] != 0.0) return fail("unseen tag", 0);
        for (int s = 0; s < K.n; s++) {
            const bool skipped = !round && (s == 3 || s == 4);
            for (int i = 0; i < 12; i++)
                if (skipped ? o.poses[12 * s + i] != K.poses0[12 * s + i] : !(std::fabs(o.poses[12 * s + i] - K.poses[12 * s + i]) < 1e-6)) return fail("pose", s);
        }
        iters = o.res.iters;
        // a subset at an offset inside a larger index array, the poses at that offset of a larger output; the position of tag 1 and
        // the rotation of tag 2 frozen, three iterations: MAXIT, and the frozen parts stay bit for bit
        std::vector<int32_t> idx2{7, 7, 0, 1, 2, 5, 6, 8, 9, 11, 3};
        const ck_rigcal_problem_t q2{8, 2};
        Capture B = K;
        B.fixed[1] = 0x38; B.fixed[2] = 0x07;
        ck_fieldcal_params_t p2 = p;
        p2.max_iters = 3;
        Out o2;
        o2.poses.assign(12 * idx2.size(), -1.0);
        rc = refine(p2, B, q2, idx2, o2);
        if (rc != CK_OK || o2.res.status != CK_CALIB_MAXIT || o2.res.iters != 3 || o2.res.n_steps != 8) return fail("maxit", rc ? rc : o2.res.status);
        if (o2.poses[0] != -1.0 || o2.poses[12 * 2 - 1] != -1.0 || o2.poses[12 * 10] != -1.0) return fail("poses outside the problem", 0);
        if (o2.sight[1] > 0 && (std::memcmp(o2.layout[1].t, B.layout0[1].t, sizeof(double) * 3) != 0 || std::memcmp(o2.layout[1].q, B.layout0[1].q, sizeof(double) * 4) == 0))
            return fail("frozen position", 1);
        if (o2.sight[2] > 0 && (std::memcmp(o2.layout[2].q, B.layout0[2].q, sizeof(double) * 4) != 0 || std::memcmp(o2.layout[2].t, B.layout0[2].t, sizeof(double) * 3) == 0))
            return fail("frozen rotation", 2);
        // the Jacobian of one sighting
        double r[12], J[4 * 36];
        const double v[12] = {0.1, -0.2, 0.97, 0.1, -0.1, 0.98, 0.2, -0.1, 0.97, 0.2, -0.2, 0.96}, P[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0.5, 0.25, 2};
        if (ck_fieldcal_jacobian(&K.mounts[0], P, &K.truth[1], v, 4, 0x7, r, J) != CK_OK || J[0] != 0 || J[1] != 0 || J[2] != 0 || J[12 + 2] != 0 || J[3] == 0) return fail("jacobian", 0);
        if (ck_fieldcal_jacobian(&K.mounts[0], P, &K.truth[1], v, 5, 0, r, J) != CK_EINVAL) return fail("jacobian n", 0);
        // the refusals, in their order: the earlier wins when two apply
        const int nt = (int)K.tag_index.size(), nb = (int)(K.bear.size() / 3);
        ck_fieldcal_params_t bad = p;
        if (check(nullptr, K, K.C, &q, idx, nt, nb) != CK_EINVAL) return fail("null", 0);
        if (check(&p, K, 0, &q, idx, nt, nb) != CK_EINVAL || check(&p, K, 9, &q, idx, nt, nb) != CK_EINVAL) return fail("n_cams", 0);
        if (check(&p, K, K.C, &q, idx, nt, nb, 0) != CK_EINVAL) return fail("n_layout", 0);
        if (check(&p, K, K.C, &q, idx, nt - 1, nb) != CK_EINVAL) return fail("tags outside", 0);
        if (check(&p, K, K.C, &q, idx, nt, nb - 1) != CK_EINVAL) return fail("bearings outside", 0);
        {
            Capture D = K;
            D.rec[1].n_bearings -= 1;
            if (check(&p, D, D.C, &q, idx, nt, nb) != CK_EINVAL) return fail("4 n_tags", 0);
        }
        if (check(&p, K, K.C, &q, idx, nt, nb, L - 2) != CK_EINVAL) return fail("tag_index out of range", 0);
        {
            std::vector<int32_t> i3 = idx;
            i3[4] = i3[3];
            if (check(&p, K, K.C, &q, i3, nt, nb) != CK_EINVAL) return fail("not increasing", 0);
            i3[4] = K.n;
            if (check(&p, K, K.C, &q, i3, nt, nb) != CK_EINVAL) return fail("step out of range", 0);
            const ck_rigcal_problem_t past{K.n, 1};
            if (check(&p, K, K.C, &past, idx, nt, nb) != CK_EINVAL) return fail("index outside", 0);
        }
        bad.max_iters = 0;
        if (check(&bad, K, K.C, &q, idx, nt, nb) != CK_EINVAL) return fail("max_iters", 0);
        bad = p; bad.max_iters = 10001;
        if (check(&bad, K, K.C, &q, idx, nt, nb) != CK_EINVAL) return fail("max_iters high", 0);
        bad = p; bad.min_steps = 0;
        if (check(&bad, K, K.C, &q, idx, nt, nb) != CK_EINVAL) return fail("min_steps", 0);
        bad = p; bad.min_tags_per_step = 1;
        if (check(&bad, K, K.C, &q, idx, nt, nb) != CK_EINVAL) return fail("min_tags_per_step", 0);
        {
            Capture D = K;
            D.fixed[3] = 64;
            if (check(&p, D, D.C, &q, idx, nt, nb) != CK_EINVAL) return fail("mask", 0);
            D = K;
            D.bear[5] = NAN;
            if (check(&p, D, D.C, &q, idx, nt, nb) != CK_EINVAL) return fail("not finite", 0);
            D = K;
            D.mounts[0].t[2] = INFINITY;
            if (check(&p, D, D.C, &q, idx, nt, nb) != CK_EINVAL) return fail("mount not finite", 0);
            D = K;
            D.layout0[L - 1].q[0] = D.layout0[L - 1].q[1] = D.layout0[L - 1].q[2] = D.layout0[L - 1].q[3] = 0;
            if (check(&p, D, D.C, &q, idx, nt, nb) != CK_EINVAL) return fail("layout not finite", 0);
            D = K;
            D.tag_index[D.rec[0].tag_offset + 1] = D.tag_index[D.rec[0].tag_offset];
            if (check(&p, D, D.C, &q, idx, nt, nb) != CK_EINVAL) return fail("duplicate tag in a view", 0);
            D = K;
            D.fixed[0] = 0x3E; D.fixed[L - 1] = CK_FIELDCAL_FIX_ALL; // the only wholly frozen tag has no sighting
            if (check(&p, D, D.C, &q, idx, nt, nb) != CK_EINVAL) return fail("gauge", 0);
        }
        {
            std::vector<int32_t> big(CK_FIELDCAL_MAX_STEPS + 1, 0);
            const ck_rigcal_problem_t qb{CK_FIELDCAL_MAX_STEPS + 1, 0};
            if (check(&p, K, K.C, &qb, big, nt, nb) != CK_EINVAL) return fail("capacity after order", 0); // (not increasing comes first)
        }
        if (check(&p, K, K.C, &q, idx, nt, nb) != CK_OK) return fail("valid", 0);
    }
    // beyond CK_FIELDCAL_MAX_STEPS: a capture of that many empty steps plus one with tags
    {
        Capture K = make(1, 3, first1, count1);
        const int n = CK_FIELDCAL_MAX_STEPS + 1;
        std::vector<ck_sqpnp_problem_t> rec((size_t)n);
        std::memset(rec.data(), 0, sizeof(ck_sqpnp_problem_t) * rec.size());
        rec[0] = K.rec[0];
        std::vector<int32_t> idx(n);
        for (int s = 0; s < n; s++) idx[s] = s;
        const ck_rigcal_problem_t q{n, 0};
        const int rc = ck_fieldcal_check(&p, 1, rec.data(), n, K.tag_index.data(), (int32_t)K.tag_index.size(), K.bear.data(), (int32_t)(K.bear.size() / 3),
                                         &q, 1, idx.data(), n, K.mounts.data(), K.layout0.data(), L, K.fixed.data());
        if (rc != CK_ECAPACITY) return fail("capacity", rc);
    }
    // beyond CK_FIELDCAL_MAX_TAGS: one view of 65 different tags of a layout of 65
    {
        const int T = CK_FIELDCAL_MAX_TAGS + 1;
        std::vector<ck_iso3_t> lay(T);
        std::vector<uint8_t> fx(T, 0);
        std::vector<int32_t> ti(T), idx{0};
        std::vector<double> bear(12 * (size_t)T, 0.5);
        for (int k = 0; k < T; k++) { std::memset(&lay[k], 0, sizeof lay[k]); lay[k].q[0] = 1; lay[k].t[0] = k; ti[k] = k; }
        fx[0] = CK_FIELDCAL_FIX_ALL;
        ck_sqpnp_problem_t rec;
        std::memset(&rec, 0, sizeof rec);
        rec.n_tags = T; rec.n_bearings = 4 * T;
        ck_iso3_t mount;
        std::memset(&mount, 0, sizeof mount);
        mount.q[0] = 1;
        const ck_rigcal_problem_t q{1, 0};
        int rc = ck_fieldcal_check(&p, 1, &rec, 1, ti.data(), T, bear.data(), 4 * T, &q, 1, idx.data(), 1, &mount, lay.data(), T, fx.data());
        if (rc != CK_ECAPACITY) return fail("tag capacity", rc);
        rec.n_tags = T - 1; rec.n_bearings = 4 * (T - 1);
        rc = ck_fieldcal_check(&p, 1, &rec, 1, ti.data(), T, bear.data(), 4 * T, &q, 1, idx.data(), 1, &mount, lay.data(), T, fx.data());
        if (rc != CK_OK) return fail("tags at the cap", rc);
    }
    std::printf("OK %d iterations\n", iters);
    return 0;
}
