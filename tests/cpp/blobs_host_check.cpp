// blobs_host_check — the host half of the coloured-piece detector (ck_blobs_host.c: ck_blob_check, ck_blob_rgb_hsv, ck_blob_mask_host,
// ck_blobs_host) alone under AddressSanitizer + UBSan, run by tests/test_blobs_host.py.  Exactly sized heap buffers, so a read or a
// write past any of them stops the program: widths around the word size, the smallest frames, full and empty masks, four classes,
// every morphology depth, the overflow rule with one slot, cap 0, a camera and a mount.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "chalkydri_hip.h"

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "blobs_host_check: %s failed at line %d\n", #c, __LINE__); return 1; } } while (0)

static uint32_t rng_state = 12345u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

int main() {
    ck_blob_params_t pp;
    ck_blob_params_default(&pp);
    REQUIRE(ck_blob_check(&pp) == CK_OK);
    REQUIRE(ck_blob_check(nullptr) == CK_EINVAL);
    long total = 0;
    const int sizes[][2] = {{1, 1}, {1, 7}, {7, 1}, {16, 16}, {31, 5}, {32, 9}, {33, 17}, {64, 3}, {65, 33}, {130, 21}};
    for (const auto &wh : sizes) {
        const int W = wh[0], H = wh[1], n = 2, ww = (W + 31) / 32;
        for (int pattern = 0; pattern < 4; pattern++) {
            std::vector<uint8_t> rgb((size_t)n * W * H * 3);
            for (size_t i = 0; i < rgb.size() / 3; i++) {
                const bool on = pattern == 0 ? (rnd() & 3) != 0 : pattern == 1 ? true : pattern == 2 ? false : ((i % W + i / W) & 1) == 0;
                rgb[3 * i] = on ? 250 : (uint8_t)(rnd() & 31); rgb[3 * i + 1] = on ? (uint8_t)(rnd() & 63) : 0; rgb[3 * i + 2] = (uint8_t)(rnd() & 15);
            }
            for (int depth = 0; depth <= 4; depth += 2) {
                ck_blob_params_default(&pp);
                pp.n_classes = 4; pp.erode = depth; pp.dilate = 4 - depth;
                pp.cls[0].h_min = 170; pp.cls[0].h_max = 10; // red wraps
                pp.cls[1].h_min = 0; pp.cls[1].h_max = 179; pp.cls[1].s_min = 0; pp.cls[1].v_min = 0; pp.cls[1].min_area = 0; // everything
                pp.cls[2].h_min = 60; pp.cls[2].h_max = 60;
                pp.cls[3].min_area = 1;
                pp.max_components = pattern == 3 ? 1 : 64;
                pp.has_camera = 1; pp.cam.model = CK_CAMERA_EUCM;
                pp.cam.k[0] = pp.cam.k[1] = 90.0; pp.cam.k[2] = W / 2.0; pp.cam.k[3] = H / 2.0; pp.cam.k[4] = 0.6; pp.cam.k[5] = 1.1;
                pp.has_mount = 1; pp.robot_to_cam.q[0] = 0.5; pp.robot_to_cam.q[1] = -0.5; pp.robot_to_cam.q[2] = 0.5; pp.robot_to_cam.q[3] = -0.5;
                pp.robot_to_cam.t[1] = 0.5;
                REQUIRE(ck_blob_check(&pp) == CK_OK);
                for (int cls = 0; cls < 4; cls++)
                    for (int stage = 0; stage < 2; stage++) {
                        std::vector<uint32_t> bits((size_t)n * H * ww);
                        REQUIRE(ck_blob_mask_host(&pp, rgb.data(), W, H, n, cls, stage, bits.data()) == CK_OK);
                        if (W & 31)
                            for (size_t r = 0; r < (size_t)n * H; r++) REQUIRE((bits[r * ww + ww - 1] >> (W & 31)) == 0);
                    }
                for (int cap : {0, 1, 5}) {
                    std::vector<ck_blob_t> out((size_t)n * 4 * cap);
                    std::vector<int32_t> counts((size_t)n * 4);
                    std::vector<uint32_t> status((size_t)n);
                    REQUIRE(ck_blobs_host(&pp, rgb.data(), W, H, n, cap ? out.data() : reinterpret_cast<ck_blob_t *>(counts.data()), cap, counts.data(),
                                          status.data()) == CK_OK);
                    for (int32_t c : counts) { REQUIRE(c >= 0 && c <= W * H); total += c; }
                }
            }
        }
    }
    std::vector<uint8_t> rgb(3 * 256), hsv(3 * 256);
    for (size_t i = 0; i < rgb.size(); i++) rgb[i] = (uint8_t)rnd();
    REQUIRE(ck_blob_rgb_hsv(rgb.data(), 256, hsv.data()) == CK_OK);
    for (int i = 0; i < 256; i++) REQUIRE(hsv[3 * i] < 180);
    REQUIRE(ck_blob_rgb_hsv(rgb.data(), 0, hsv.data()) == CK_OK);
    std::printf("blobs_host_check ok: %ld targets counted\n", total);
    return 0;
}
