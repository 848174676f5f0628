// subpix_host_check — the host half of the sub-pixel corners (ck_subpix_host.c: ck_subpix_weights, ck_corner_subpix_host,
// ck_board_corners_host) under AddressSanitizer and UBSan, driven from tests/test_subpix_host.py.  Stand-alone: it links the one C
// file, not the library, and needs no device.  The frames are allocated at their exact size (a strided one too), so that a sample
// past a frame's last pixel is seen: points on the frame border and in its corners, windows that hang over every edge, w = 2 and
// w = 7, n = 0, estimates that run away, a board whose tags reach the frame edge, and the refusals.
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

// a checkerboard of `cell`-pixel squares: every crossing is an X-saddle
static std::vector<uint8_t> checker(int w, int h, int stride, int cell, int ox, int oy) {
    std::vector<uint8_t> px((size_t)stride * h, 0);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) px[(size_t)y * stride + x] = (((x + ox) / cell + (y + oy) / cell) & 1) ? 210 : 30;
    return px;
}

int main() {
    const int W = 97, H = 61;
    std::vector<uint8_t> a = checker(W, H, W, 12, 0, 0), b = checker(W, H, W + 7, 9, 3, 5);
    b.resize((size_t)(W + 7) * (H - 1) + W); // the strided frame ends with its last pixel
    ck_image_u8_t imgs[2] = {{a.data(), W, H, W}, {b.data(), W, H, W + 7}};
    std::vector<double> pts;
    std::vector<int32_t> fr;
    for (int y = 0; y <= H; y += 6)
        for (int x = 0; x <= W; x += 8) { pts.push_back(x == W ? W : x + 0.3); pts.push_back(y > H - 6 ? H : y + 0.45); fr.push_back((x / 8 + y / 6) & 1); }
    const double corners[][2] = {{0, 0}, {W, 0}, {0, H}, {W, H}, {0.5, 0.5}, {W - 0.5, H - 0.5}, {12.0, 12.0}, {48.2, 35.6}};
    for (auto &c : corners) { pts.push_back(c[0]); pts.push_back(c[1]); fr.push_back(0); }
    const int n = (int)fr.size();
    std::vector<double> out(2 * n);
    std::vector<ck_subpix_info_t> info(n);
    ck_subpix_params_t pp;
    for (int w : {2, 5, 7}) {
        ck_subpix_params_default(&pp);
        pp.half_win = w;
        std::vector<double> wts((size_t)(2 * w + 1) * (2 * w + 1)); // exactly the table's size
        if (ck_subpix_weights(&pp, wts.data()) != CK_OK) return fail("weights", w);
        if (wts[(size_t)w * (2 * w + 1) + w] != 1.0 || wts[0] != wts.back()) return fail("weights centre", w);
        if (ck_corner_subpix_host(&pp, imgs, 2, fr.data(), pts.data(), n, out.data(), info.data()) != CK_OK) return fail("refine", w);
        int conv = 0;
        for (int i = 0; i < n; i++) {
            if (info[i].status < CK_SUBPIX_CONVERGED || info[i].status > CK_SUBPIX_REJECTED) return fail("status", i);
            if (!std::isfinite(out[2 * i]) || !std::isfinite(out[2 * i + 1])) return fail("not finite", i);
            const bool same = std::memcmp(&out[2 * i], &pts[2 * i], 16) == 0;
            if ((info[i].status == CK_SUBPIX_FLAT || info[i].status == CK_SUBPIX_REJECTED) && !same) return fail("input not returned", i);
            if (std::fabs(out[2 * i] - pts[2 * i]) > w || std::fabs(out[2 * i + 1] - pts[2 * i + 1]) > w) return fail("moved too far", i);
            conv += info[i].status == CK_SUBPIX_CONVERGED;
        }
        if (conv < 8) return fail("few converged", conv);
        if (info[n - 1].status != CK_SUBPIX_CONVERGED || std::fabs(out[2 * n - 2] - 48.0) > 0.05 || std::fabs(out[2 * n - 1] - 36.0) > 0.05)
            return fail("the crossing at (48, 36)", info[n - 1].status);
        // eps = 0, one and many steps, info NULL, frame NULL
        pp.eps = 0.0; pp.max_iters = 1;
        if (ck_corner_subpix_host(&pp, imgs, 1, nullptr, pts.data() + 2 * (n - 8), 8, out.data(), nullptr) != CK_OK) return fail("frame null", w);
        pp.max_iters = 1000; pp.det_min = 0.0; // (nothing is FLAT but an exact zero: estimates may run away, and are rejected)
        if (ck_corner_subpix_host(&pp, imgs, 2, fr.data(), pts.data(), n, out.data(), info.data()) != CK_OK) return fail("long", w);
        for (int i = 0; i < n; i++)
            if (!std::isfinite(out[2 * i]) || !std::isfinite(out[2 * i + 1])) return fail("long not finite", i);
    }
    ck_subpix_params_default(&pp);
    if (ck_corner_subpix_host(&pp, imgs, 2, fr.data(), pts.data(), 0, nullptr, nullptr) != CK_OK) return fail("n = 0", 0);
    if (ck_corner_subpix_host(&pp, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr) != CK_OK) return fail("n = 0, no images", 0);
    // refusals
    const double nan = std::numeric_limits<double>::quiet_NaN(), bad_pts[][2] = {{nan, 1}, {1, -0.5}, {W + 0.25, 1}, {1, H + 1.0}};
    for (auto &p : bad_pts)
        if (ck_corner_subpix_host(&pp, imgs, 2, nullptr, p, 1, out.data(), nullptr) != CK_EINVAL) return fail("bad point", 0);
    const int32_t bad_fr[2] = {2, -1};
    for (int i = 0; i < 2; i++)
        if (ck_corner_subpix_host(&pp, imgs, 2, &bad_fr[i], pts.data(), 1, out.data(), nullptr) != CK_EINVAL) return fail("bad frame", i);
    ck_subpix_params_t q = pp;
    q.half_win = 8;
    if (ck_subpix_weights(&q, out.data()) != CK_EINVAL || ck_corner_subpix_host(&q, imgs, 2, nullptr, pts.data(), 1, out.data(), nullptr) != CK_EINVAL)
        return fail("half_win 8", 0);
    q = pp; q.half_win = 1;
    if (ck_subpix_weights(&q, out.data()) != CK_EINVAL) return fail("half_win 1", 0);

    // a board of 12-pixel "tags" without spacing on the checkerboard: its crossings are the tags' corners, the outer ones lie on or
    // near the frame edge, so predictions are skipped there and the rest is refined; one seed in the middle
    ck_board_t board = {5, 8, 10, 0, 1.0, 0.0};
    ck_board_params_t bp;
    ck_board_params_default(&bp);
    std::vector<ck_detection_t> dets(3);
    std::memset(dets.data(), 0, sizeof(ck_detection_t) * dets.size());
    const int r = 2, c = 3;
    dets[0].id = 10 + r * 8 + c; // corners: bottom-left, bottom-right, top-right, top-left
    const double x0 = 12.0 * c + 0.3, x1 = 12.0 * (c + 1) - 0.2, y0 = 12.0 * r + 0.25, y1 = 12.0 * (r + 1) - 0.3;
    const double p[4][2] = {{x0, y1}, {x1, y1}, {x1, y0}, {x0, y0}};
    std::memcpy(dets[0].p, p, sizeof p);
    dets[1] = dets[0]; dets[1].p[0][0] += 5; // the same id again: not looked at
    dets[2] = dets[0]; dets[2].id = 9;       // not on the board
    const int32_t counts[2] = {3, 0};
    ck_image_u8_t two[2] = {imgs[0], imgs[0]};
    const int nt = board.rows * board.cols;
    std::vector<double> uv((size_t)2 * nt * 8);
    std::vector<uint8_t> state((size_t)2 * nt);
    int32_t n_tags[2] = {-1, -1};
    pp.half_win = 3; // (12-pixel squares: the window must not reach the next crossing)
    if (ck_board_corners_host(&board, &pp, &bp, two, 2, dets.data(), 3, counts, uv.data(), state.data(), n_tags) != CK_OK) return fail("board", 0);
    if (state[(size_t)r * 8 + c] != 1) return fail("seed", state[(size_t)r * 8 + c]);
    int known = 0;
    for (int t = 0; t < nt; t++) {
        known += state[t] != 0;
        if (state[nt + t]) return fail("tag in the empty frame", t);
        for (int k = 0; k < 4 && state[t]; k++) {
            const double u = uv[(size_t)t * 8 + 2 * k], v = uv[(size_t)t * 8 + 2 * k + 1];
            if (std::fabs(u - std::round(u / 12) * 12) > 0.05 || std::fabs(v - std::round(v / 12) * 12) > 0.05) return fail("corner off its crossing", t);
        }
    }
    if (known != n_tags[0] || n_tags[1] != 0) return fail("n_tags", n_tags[0]);
    if (known < 6) return fail("few tags recovered", known);
    board.rows = 9;
    if (ck_board_corners_host(&board, &pp, &bp, two, 2, dets.data(), 3, counts, uv.data(), state.data(), n_tags) != CK_EINVAL) return fail("72 tags", 0);
    std::printf("subpix_host_check ok: %d points x 3 windows, board %d tags known\n", n, known);
    return 0;
}
