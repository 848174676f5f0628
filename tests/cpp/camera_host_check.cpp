// camera_host_check — the host half of the camera models (ck_camera_host.c: ck_camera_check, ck_camera_unproject_host,
// ck_camera_normalize_host, ck_camera_project_host) under AddressSanitizer and UBSan, driven from tests/test_camera_host.py.
// Stand-alone: it links the one C file, not the library, and needs no device.  Walks a pixel grid through the three models (an odd
// count, so that a write past the arrays' ends is seen), the round trip, the valid disc, the exact identities and the refusals.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "chalkydri_hip.h"

static int fail(const char *what, int v) {
    std::printf("FAIL %s %d\n", what, v);
    return 1;
}

static ck_camera_t camera(int model, double fx, double fy, double cx, double cy, double a = 0, double b = 0) {
    ck_camera_t c;
    std::memset(&c, 0, sizeof c);
    c.model = model;
    c.k[0] = fx; c.k[1] = fy; c.k[2] = cx; c.k[3] = cy; c.k[4] = a; c.k[5] = b;
    return c;
}

int main() {
    const int W = 1280, H = 800;
    std::vector<double> px;
    for (int y = 0; y <= H; y += 37)
        for (int x = 0; x <= W; x += 41) { px.push_back(x); px.push_back(y); }
    const int n = (int)(px.size() / 2);
    std::vector<double> b(3 * n), back(2 * n), xy(2 * n);
    std::vector<uint8_t> ok(n), ok2(n);
    const ck_camera_t eucm = camera(CK_CAMERA_EUCM, 500, 502, 640, 400, 0.62, 1.08);
    const ck_camera_t ucm = camera(CK_CAMERA_UCM, 700, 700, 630, 410, 0.55, 123.0); // (k[5] is not looked at)
    ck_camera_t cv5 = camera(CK_CAMERA_OPENCV5, 900, 905, 640, 400, -0.03, 0.002);
    cv5.k[6] = 1e-3; cv5.k[7] = -2e-4; cv5.k[8] = 0.01;
    const ck_camera_t *all[3] = {&eucm, &ucm, &cv5};
    for (const ck_camera_t *c : all) {
        if (ck_camera_check(c) != CK_OK) return fail("check", c->model);
        if (ck_camera_unproject_host(c, px.data(), n, b.data(), ok.data()) != CK_OK) return fail("unproject", c->model);
        if (ck_camera_project_host(c, b.data(), n, back.data(), ok2.data()) != CK_OK) return fail("project", c->model);
        if (ck_camera_normalize_host(c, px.data(), n, xy.data(), ok2.data()) != CK_OK) return fail("normalize", c->model);
        for (int i = 0; i < n; i++) {
            if (!ok[i]) return fail("grid pixel not ok", i);
            const double nn = b[3 * i] * b[3 * i] + b[3 * i + 1] * b[3 * i + 1] + b[3 * i + 2] * b[3 * i + 2];
            if (!(std::fabs(nn - 1.0) < 1e-14)) return fail("unit bearing", i);
            if (!(std::fabs(back[2 * i] - px[2 * i]) < 1e-8) || !(std::fabs(back[2 * i + 1] - px[2 * i + 1]) < 1e-8)) return fail("round trip", i);
        }
    }
    // UCM(alpha) = EUCM(alpha, 1.0), byte for byte
    {
        const ck_camera_t e1 = camera(CK_CAMERA_EUCM, 700, 700, 630, 410, 0.55, 1.0);
        std::vector<double> b1(3 * n);
        ck_camera_unproject_host(&ucm, px.data(), n, b.data(), ok.data());
        ck_camera_unproject_host(&e1, px.data(), n, b1.data(), ok2.data());
        if (std::memcmp(b.data(), b1.data(), sizeof(double) * 3 * n) != 0 || ok != ok2) return fail("ucm is eucm beta 1", 0);
    }
    // alpha = 0 = the zero-distortion OpenCVModel5, byte for byte
    {
        const ck_camera_t e0 = camera(CK_CAMERA_EUCM, 600, 610, 640, 400, 0.0, 1.3), p0 = camera(CK_CAMERA_OPENCV5, 600, 610, 640, 400);
        std::vector<double> b1(3 * n);
        ck_camera_unproject_host(&e0, px.data(), n, b.data(), ok.data());
        ck_camera_unproject_host(&p0, px.data(), n, b1.data(), ok2.data());
        if (std::memcmp(b.data(), b1.data(), sizeof(double) * 3 * n) != 0 || ok != ok2) return fail("alpha 0 is the pinhole", 0);
    }
    // the valid disc: r2 >= 1 / (beta (2 alpha - 1)) is not ok
    {
        const double r = std::sqrt(1.0 / (1.08 * (2 * 0.62 - 1.0)));
        const double p[4] = {640 + 500 * r * 1.001, 400, 640 + 500 * r * 0.999, 400};
        double bb[6], q[4];
        uint8_t o[2];
        if (ck_camera_unproject_host(&eucm, p, 2, bb, o) != CK_OK || o[0] != 0 || o[1] != 1) return fail("disc", o[0] * 2 + o[1]);
        if (!(bb[5] < 0.0)) return fail("inside the disc, behind the image plane", 0);
        if (ck_camera_normalize_host(&eucm, p, 2, q, o) != CK_OK || o[0] != 0 || o[1] != 0) return fail("no normalised point", 0);
        const double behind[6] = {0.1, 0.0, -1.0, 0.0, 0.0, 1.0};
        if (ck_camera_project_host(&eucm, behind, 2, q, o) != CK_OK || o[0] != 0 || o[1] != 1) return fail("cone", 0);
    }
    // n = 0 touches nothing
    if (ck_camera_unproject_host(&eucm, px.data(), 0, b.data(), ok.data()) != CK_OK) return fail("n 0", 0);
    // refusals
    ck_camera_t bad = eucm;
    if (ck_camera_check(nullptr) != CK_EINVAL) return fail("null", 0);
    bad.model = 3;
    if (ck_camera_check(&bad) != CK_EINVAL) return fail("model", 0);
    bad = eucm; bad.k[2] = std::numeric_limits<double>::quiet_NaN();
    if (ck_camera_check(&bad) != CK_EINVAL) return fail("nan", 0);
    bad = eucm; bad.k[0] = 0.0;
    if (ck_camera_check(&bad) != CK_EINVAL) return fail("fx", 0);
    bad = eucm; bad.k[4] = 1.01;
    if (ck_camera_check(&bad) != CK_EINVAL) return fail("alpha", 0);
    bad = eucm; bad.k[5] = 0.0;
    if (ck_camera_check(&bad) != CK_EINVAL) return fail("beta", 0);
    bad = eucm; bad.k[7] = 1e-9;
    if (ck_camera_check(&bad) != CK_EINVAL) return fail("unused slot", 0);
    if (ck_camera_unproject_host(&eucm, nullptr, n, b.data(), ok.data()) != CK_EINVAL) return fail("null px", 0);
    if (ck_camera_project_host(&eucm, b.data(), -1, back.data(), ok.data()) != CK_EINVAL) return fail("negative n", 0);
    std::printf("OK %d pixels\n", n);
    return 0;
}
