// rig_host_check — the host twin of the camera-rig solver (ck_rig_host.c: ck_rig_params_default, ck_rig_solve_host) under
// AddressSanitizer and UBSan, driven from tests/test_cpp_rig.py.  Stand-alone: it links the one C file, not the library, and needs no
// device.  Solves 20 random noise-free rigs of 1..4 cameras (a camera may see nothing) in one call and compares with the truth, then
// walks the edge cases: a step without tags, a camera without tags, the refusals.  Prints OK.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "chalkydri_hip.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double uniform(double lo, double hi) { // xorshift64*
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    const uint64_t r = rng_state * 0x2545F4914F6CDD1Dull;
    return lo + (hi - lo) * (double)(r >> 11) / 9007199254740992.0;
}
struct Mat { double m[9]; };
static Mat quat_mat(const double q[4]) {
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    return {{1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
             2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)}};
}
static void random_quat(double q[4], double spread) { // spread 1: any rotation; small: near the identity
    double n = 0;
    q[0] = spread >= 1 ? uniform(-1, 1) : 1.0;
    for (int k = 1; k < 4; k++) q[k] = uniform(-1, 1) * spread;
    for (int k = 0; k < 4; k++) n += q[k] * q[k];
    n = std::sqrt(n);
    if (n < 1e-3) { q[0] = 1; q[1] = q[2] = q[3] = 0; n = 1; }
    for (int k = 0; k < 4; k++) q[k] /= n;
}
static void mul(const Mat &A, const double v[3], double o[3]) {
    for (int i = 0; i < 3; i++) o[i] = A.m[i * 3] * v[0] + A.m[i * 3 + 1] * v[1] + A.m[i * 3 + 2] * v[2];
}
static void mul_t(const Mat &A, const double v[3], double o[3]) {
    for (int i = 0; i < 3; i++) o[i] = A.m[i] * v[0] + A.m[3 + i] * v[1] + A.m[6 + i] * v[2];
}

static int fail(const char *what, int v) {
    std::printf("FAIL %s %d\n", what, v);
    return 1;
}

int main() {
    ck_rig_params_t prm;
    ck_rig_params_default(&prm);
    if (prm.sqpnp.max_iter != 15 || prm.sqpnp.tol_sq != 1e-16 || prm.sign_change_error != 600.0 || prm.rig_id != 255) return fail("defaults", 0);
    const int N = 20, CAMS = 4;
    std::vector<ck_sqpnp_problem_t> probs((size_t)CAMS * N);
    std::vector<ck_iso3_t> tags;
    std::vector<double> bearings, gyro(N), truth_yaw(N), truth_pos(3 * N);
    const double S = 0.1651 / 2, corners[4][3] = {{0, -S, -S}, {0, S, -S}, {0, S, S}, {0, -S, S}};
    for (int s = 0; s < N; s++) {
        const double yaw = uniform(-3.1, 3.1), twr[3] = {uniform(2, 14), uniform(1, 7), 0};
        const Mat Rwr = {{std::cos(yaw), -std::sin(yaw), 0, std::sin(yaw), std::cos(yaw), 0, 0, 0, 1}};
        gyro[s] = truth_yaw[s] = yaw;
        for (int k = 0; k < 3; k++) truth_pos[3 * s + k] = twr[k];
        const int active = 1 + (s % CAMS); // cameras past it see nothing at this step
        for (int c = 0; c < CAMS; c++) {
            ck_sqpnp_problem_t &p = probs[(size_t)c * N + s];
            std::memset(&p, 0, sizeof p);
            random_quat(p.robot_to_cam.q, 1.0);
            const Mat A = quat_mat(p.robot_to_cam.q);
            const double mount[3] = {uniform(-0.4, 0.4), uniform(-0.4, 0.4), uniform(-0.4, 0.4)};
            double am[3];
            mul(A, mount, am);
            for (int k = 0; k < 3; k++) p.robot_to_cam.t[k] = -am[k];
            p.tag_offset = (int32_t)tags.size();
            p.bearing_offset = (int32_t)(bearings.size() / 3);
            p.n_tags = c < active ? 1 + ((s + c) % 3) : 0;
            p.n_bearings = 4 * p.n_tags;
            for (int t = 0; t < p.n_tags; t++) {
                // the tag's centre 1..5 m in front of the camera; camera -> robot -> world
                const double z = uniform(1, 5), pc[3] = {uniform(-0.4, 0.4) * z, uniform(-0.3, 0.3) * z, z};
                double d[3], pr[3], pw[3];
                for (int k = 0; k < 3; k++) d[k] = pc[k] - p.robot_to_cam.t[k];
                mul_t(A, d, pr);
                mul(Rwr, pr, pw);
                ck_iso3_t tag;
                for (int k = 0; k < 3; k++) tag.t[k] = pw[k] + twr[k];
                random_quat(tag.q, 1.0);
                const Mat Rt = quat_mat(tag.q);
                tags.push_back(tag);
                for (int j = 0; j < 4; j++) { // corner -> world -> robot -> camera, the bearing is its direction
                    double cw[3], rel[3], prr[3], pcam[3];
                    mul(Rt, corners[j], cw);
                    for (int k = 0; k < 3; k++) rel[k] = cw[k] + tag.t[k] - twr[k];
                    mul_t(Rwr, rel, prr);
                    mul(A, prr, pcam);
                    for (int k = 0; k < 3; k++) pcam[k] += p.robot_to_cam.t[k];
                    const double nrm = std::sqrt(pcam[0] * pcam[0] + pcam[1] * pcam[1] + pcam[2] * pcam[2]);
                    for (int k = 0; k < 3; k++) bearings.push_back(pcam[k] / nrm);
                }
            }
        }
    }
    const int32_t nt = (int32_t)tags.size(), nb = (int32_t)(bearings.size() / 3);
    std::vector<ck_rig_result_t> res(N);
    int rc = ck_rig_solve_host(&prm, CAMS, probs.data(), N, tags.data(), nt, bearings.data(), nb, gyro.data(), res.data());
    if (rc != CK_OK) return fail("solve", rc);
    for (int s = 0; s < N; s++) {
        const ck_rig_result_t &r = res[s];
        if (!r.valid) return fail("valid", s);
        int want_tags = 0;
        for (int c = 0; c < CAMS; c++) {
            want_tags += probs[(size_t)c * N + s].n_tags;
            if (r.cam_tags[c] != probs[(size_t)c * N + s].n_tags || !(r.cam_rms[c] < 1e-6)) return fail("camera", s * 10 + c);
        }
        if (r.n_tags != want_tags) return fail("n_tags", s);
        for (int k = 0; k < 3; k++)
            if (!(std::fabs(r.pos[k] - truth_pos[3 * s + k]) < 1e-6)) return fail("pos", s);
        if (!(std::fabs(std::remainder(r.yaw - truth_yaw[s], 2 * 3.14159265358979323846)) < 1e-6)) return fail("yaw", s);
    }
    // one camera alone (the first record of camera 0 as a one-step problem at its offsets inside the larger arrays)
    ck_rig_result_t one;
    rc = ck_rig_solve_host(&prm, 1, &probs[0], 1, tags.data(), nt, bearings.data(), nb, gyro.data(), &one);
    if (rc != CK_OK || !one.valid || one.cam_tags[0] != probs[0].n_tags || one.cam_tags[1] != 0) return fail("one camera", rc);
    // a step without tags: zeroed record; no steps at all: nothing written
    ck_sqpnp_problem_t none[2];
    std::memset(none, 0, sizeof none);
    none[0].robot_to_cam.q[0] = none[1].robot_to_cam.q[0] = 1;
    ck_rig_result_t zero, blank;
    std::memset(&blank, 0, sizeof blank);
    std::memset(&zero, 0xFF, sizeof zero);
    rc = ck_rig_solve_host(&prm, 2, none, 1, nullptr, 0, nullptr, 0, gyro.data(), &zero);
    if (rc != CK_OK || std::memcmp(&zero, &blank, sizeof zero) != 0) return fail("no tags", rc);
    if (ck_rig_solve_host(&prm, 2, none, 0, nullptr, 0, nullptr, 0, gyro.data(), &zero) != CK_OK) return fail("no steps", 0);
    // refusals
    if (ck_rig_solve_host(&prm, 0, probs.data(), N, tags.data(), nt, bearings.data(), nb, gyro.data(), res.data()) != CK_EINVAL) return fail("n_cams 0", 0);
    if (ck_rig_solve_host(&prm, 9, probs.data(), N, tags.data(), nt, bearings.data(), nb, gyro.data(), res.data()) != CK_EINVAL) return fail("n_cams 9", 0);
    if (ck_rig_solve_host(nullptr, CAMS, probs.data(), N, tags.data(), nt, bearings.data(), nb, gyro.data(), res.data()) != CK_EINVAL) return fail("null", 0);
    if (ck_rig_solve_host(&prm, CAMS, probs.data(), N, nullptr, nt, bearings.data(), nb, gyro.data(), res.data()) != CK_EINVAL) return fail("null tags", 0);
    if (ck_rig_solve_host(&prm, CAMS, probs.data(), N, tags.data(), nt - 1, bearings.data(), nb, gyro.data(), res.data()) != CK_EINVAL) return fail("tags short", 0);
    if (ck_rig_solve_host(&prm, CAMS, probs.data(), N, tags.data(), nt, bearings.data(), nb - 1, gyro.data(), res.data()) != CK_EINVAL) return fail("bearings short", 0);
    ck_sqpnp_problem_t keep = probs[0];
    probs[0].n_bearings -= 1;
    if (ck_rig_solve_host(&prm, CAMS, probs.data(), N, tags.data(), nt, bearings.data(), nb, gyro.data(), res.data()) != CK_EINVAL) return fail("count", 0);
    probs[0] = keep; probs[0].tag_offset = -1;
    if (ck_rig_solve_host(&prm, CAMS, probs.data(), N, tags.data(), nt, bearings.data(), nb, gyro.data(), res.data()) != CK_EINVAL) return fail("offset", 0);
    probs[0] = keep;
    std::printf("OK %d rigs\n", N);
    return 0;
}
