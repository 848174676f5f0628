// calib_host_check — the host half of the camera calibration (ck_calib_host.c: ck_calib_check, ck_calib_init, ck_calib_refine_host)
// under AddressSanitizer and UBSan, driven from tests/test_cpp_calib.py.  Stand-alone: it links the one C file, not the library,
// and needs no device.  Makes one F = 4 case of a 6 x 6 board seen by a mildly distorted camera, solves it, solves it again with a
// ragged subset and with frozen distortion, walks the refusals, and prints OK.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "chalkydri_hip.h"

static void project(const double *k, const double *P, double X, double Y, double *u, double *v) {
    const double px = P[0] * X + P[1] * Y + P[9], py = P[3] * X + P[4] * Y + P[10], pz = P[6] * X + P[7] * Y + P[11];
    const double x = px / pz, y = py / pz, r2 = x * x + y * y, rad = 1 + r2 * (k[4] + r2 * (k[5] + r2 * k[8]));
    *u = k[0] * (x * rad + 2 * k[6] * x * y + k[7] * (r2 + 2 * x * x)) + k[2];
    *v = k[1] * (y * rad + k[6] * (r2 + 2 * y * y) + 2 * k[7] * x * y) + k[3];
}

static int fail(const char *what, int v) {
    std::printf("FAIL %s %d\n", what, v);
    return 1;
}

int main() {
    const double k[9] = {1368.33, 1368.51, 784.10, 655.20, -0.0343, -0.0021, -0.001, -0.00014, 0.0153};
    const int W = 1600, H = 1304, F = 4;
    // poses: Rz(spin) Rx(tilt_x) Ry(tilt_y), board centre about 0.6 m away
    const double spin[F] = {0.3, 2.1, -1.2, 3.0}, tx[F] = {0.35, -0.3, 0.1, 0.45}, ty[F] = {-0.2, 0.4, 0.5, -0.35}, dist[F] = {0.6, 0.75, 0.55, 0.8};
    const double off[F][2] = {{-0.05, 0.02}, {0.08, -0.04}, {0.0, 0.06}, {-0.07, -0.05}};
    std::vector<double> bxy, uv;
    std::vector<int32_t> starts{0};
    const double pitch = 0.088 * 1.3, s = 0.044, c0 = (5 * pitch + 0.088) / 2;
    for (int f = 0; f < F; f++) {
        const double cz = std::cos(spin[f]), sz = std::sin(spin[f]), cx = std::cos(tx[f]), sx = std::sin(tx[f]), cy = std::cos(ty[f]), sy = std::sin(ty[f]);
        const double Rz[9] = {cz, -sz, 0, sz, cz, 0, 0, 0, 1}, Rx[9] = {1, 0, 0, 0, cx, -sx, 0, sx, cx}, Ry[9] = {cy, 0, sy, 0, 1, 0, -sy, 0, cy};
        double A[9], P[12];
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) A[3 * i + j] = Rx[3 * i] * Ry[j] + Rx[3 * i + 1] * Ry[3 + j] + Rx[3 * i + 2] * Ry[6 + j];
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) P[3 * i + j] = A[3 * i] * Rz[j] + A[3 * i + 1] * Rz[3 + j] + A[3 * i + 2] * Rz[6 + j];
        const double ctr[3] = {off[f][0], off[f][1], dist[f]};
        for (int i = 0; i < 3; i++) P[9 + i] = ctr[i] - (P[3 * i] * c0 + P[3 * i + 1] * c0);
        for (int t = 0; t < 36; t++)
            for (int c = 0; c < 4; c++) {
                static const double d[4][2] = {{-1, 1}, {1, 1}, {1, -1}, {-1, -1}};
                const double X = (t % 6) * pitch + s + d[c][0] * s, Y = (t / 6) * pitch + s + d[c][1] * s;
                double u, v;
                project(k, P, X, Y, &u, &v);
                if (u < 4 || u > W - 5 || v < 4 || v > H - 5) continue;
                bxy.push_back(X); bxy.push_back(Y); uv.push_back(u); uv.push_back(v);
            }
        starts.push_back((int32_t)(bxy.size() / 2));
    }
    const int32_t n_pts = starts.back();
    ck_calib_params_t p;
    ck_calib_params_default(&p, W, H);
    if (p.max_iters != 100 || p.min_points_per_frame != 24 || p.min_frames != 3 || p.fixed_mask != 0) return fail("defaults", 0);
    const ck_calib_problem_t q{F, 0, 0, 0};
    ck_opencv5_t cam0;
    std::vector<double> poses0(12 * F), poses(12 * F);
    int32_t st = -1;
    int rc = ck_calib_init(&p, &q, bxy.data(), uv.data(), starts.data(), n_pts, F + 1, F, &cam0, poses0.data(), &st);
    if (rc != CK_OK || st != CK_CALIB_CONVERGED) return fail("init", rc ? rc : st);
    ck_calib_result_t res;
    rc = ck_calib_refine_host(&p, &q, bxy.data(), uv.data(), starts.data(), n_pts, F + 1, F, &cam0, poses0.data(), &res, poses.data());
    if (rc != CK_OK || res.status != CK_CALIB_CONVERGED) return fail("refine", rc ? rc : res.status);
    const double *got = &res.cam.fx;
    for (int i = 0; i < 9; i++)
        if (!(std::fabs(got[i] - k[i]) < 1e-6)) return fail("parameter", i);
    if (res.n_frames != F || res.n_points != n_pts || !(res.rms < 1e-9) || !(res.cost <= res.cost0)) return fail("record", res.iters);
    // in place, frozen distortion at the truth, three iterations: MAXIT, the frozen values bit-unchanged
    p.fixed_mask = CK_CALIB_FIX_DISTORTION; p.max_iters = 3;
    ck_opencv5_t cam1 = cam0;
    cam1.k1 = k[4]; cam1.k2 = k[5]; cam1.p1 = k[6]; cam1.p2 = k[7]; cam1.k3 = k[8];
    poses = poses0;
    rc = ck_calib_refine_host(&p, &q, bxy.data(), uv.data(), starts.data(), n_pts, F + 1, F, &cam1, poses.data(), &res, poses.data());
    if (rc != CK_OK || res.status != CK_CALIB_MAXIT || res.iters != 3) return fail("maxit", rc ? rc : res.status);
    if (std::memcmp(&res.cam.k1, &cam1.k1, 5 * sizeof(double)) != 0) return fail("frozen", 0);
    // a problem at offsets inside larger arrays: frames 1..3
    p.fixed_mask = 0; p.max_iters = 100;
    const ck_calib_problem_t q3{3, 1, 0, 1};
    rc = ck_calib_init(&p, &q3, bxy.data(), uv.data(), starts.data(), n_pts, F + 1, F, &cam0, poses0.data(), &st);
    if (rc != CK_OK || st != CK_CALIB_CONVERGED) return fail("init3", rc ? rc : st);
    rc = ck_calib_refine_host(&p, &q3, bxy.data(), uv.data(), starts.data(), n_pts, F + 1, F, &cam0, poses0.data(), &res, poses.data());
    if (rc != CK_OK || res.n_frames != 3 || res.n_points != starts[4] - starts[1]) return fail("refine3", rc);
    // refusals
    ck_calib_params_t bad = p;
    bad.max_iters = 0;
    if (ck_calib_check(&bad, &q, 1, bxy.data(), uv.data(), starts.data(), n_pts, F + 1, F) != CK_EINVAL) return fail("max_iters", 0);
    bad = p; bad.width = 8;
    if (ck_calib_check(&bad, &q, 1, bxy.data(), uv.data(), starts.data(), n_pts, F + 1, F) != CK_EINVAL) return fail("width", 0);
    if (ck_calib_check(&p, &q, 1, bxy.data(), uv.data(), starts.data(), n_pts - 1, F + 1, F) != CK_EINVAL) return fail("points", 0);
    if (ck_calib_check(&p, &q, 1, bxy.data(), uv.data(), starts.data(), n_pts, F, F) != CK_EINVAL) return fail("starts", 0);
    if (ck_calib_check(&p, nullptr, 1, bxy.data(), uv.data(), starts.data(), n_pts, F + 1, F) != CK_EINVAL) return fail("null", 0);
    const ck_calib_problem_t big{CK_CALIB_MAX_FRAMES + 1, 0, 0, 0};
    if (ck_calib_check(&p, &big, 1, bxy.data(), uv.data(), starts.data(), n_pts, F + 1, F) != CK_ECAPACITY) return fail("capacity", 0);
    std::printf("OK %d iterations\n", res.iters);
    return 0;
}
