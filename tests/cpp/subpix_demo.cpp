// subpix_demo — the C++ host layer's sub-pixel corners (include/chalkydri.hpp: corner_subpix, corner_subpix_host,
// Handle::set_corner_subpix, board_corners, Calibrator(recover)) driven from tests/test_cpp_subpix.py.
//   subpix_demo host W H N HALF FRAMES POINTS OUT
//       FRAMES holds N frames [H][W] of 8-bit luma; POINTS int32 n, int32 frame[n], double xy[n][2]; OUT gets xy_out [n][2] and the
//       ck_subpix_info_t records [n] of corner_subpix_host (no GPU needed)
//   subpix_demo device W H N HALF FRAMES POINTS OUT
//       the same through ck_upload_frames and corner_subpix on the device
//   subpix_demo detect W H N HALF FRAMES OUT
//       detects the N frames with Handle::set_corner_subpix(HALF) on (HALF 0: off); OUT gets int32 counts [N] and the
//       ck_detection_t records [N][64]
//   subpix_demo board W H N ROWS COLS FRAMES OUT
//       detects the N frames and recovers a ROWS x COLS board (first id 0, the default tag size and spacing) with board_corners; OUT
//       gets uv [N][ROWS * COLS][4][2], state [N][ROWS * COLS] and n_tags [N]; then a Calibrator with recover on and one with it off
//       process the frames with min_corners 4: prints "FRAMES r p" (frames each kept)
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>

#include "chalkydri.hpp"

static std::vector<uint8_t> slurp(const char *path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
template <typename T>
static void put(std::ofstream &o, const std::vector<T> &v) { o.write(reinterpret_cast<const char *>(v.data()), (std::streamsize)(v.size() * sizeof(T))); }

int main(int argc, char **argv) {
    try {
        const std::string cmd = argc > 1 ? argv[1] : "";
        if (argc < 8) { std::fprintf(stderr, "usage: see the head of tests/cpp/subpix_demo.cpp\n"); return 2; }
        const int w = std::atoi(argv[2]), h = std::atoi(argv[3]), n = std::atoi(argv[4]);
        const bool board = cmd == "board";
        std::vector<uint8_t> px = slurp(argv[board ? 7 : 6]);
        if (n < 1 || px.size() != (size_t)w * h * n) { std::fprintf(stderr, "frames: wrong size\n"); return 2; }
        std::vector<ck_image_u8_t> imgs;
        for (int i = 0; i < n; i++) imgs.push_back({px.data() + (size_t)i * w * h, w, h, w});
        if ((cmd == "host" || cmd == "device") && argc == 9) {
            const ck_subpix_params_t pp = chalkydri::subpix_params(std::atoi(argv[5]));
            const std::vector<uint8_t> in = slurp(argv[7]);
            int32_t np = 0;
            if (in.size() >= 4) std::memcpy(&np, in.data(), 4);
            if (np < 0 || in.size() != 4 + (size_t)np * 20) { std::fprintf(stderr, "points: wrong size\n"); return 2; }
            std::vector<int32_t> fr((size_t)np);
            std::vector<double> xy((size_t)np * 2);
            std::memcpy(fr.data(), in.data() + 4, (size_t)np * 4);
            std::memcpy(xy.data(), in.data() + 4 + (size_t)np * 4, (size_t)np * 16);
            std::vector<ck_subpix_info_t> info;
            std::vector<double> out;
            if (cmd == "host") {
                out = chalkydri::corner_subpix_host(pp, imgs, fr, xy, &info);
            } else {
                chalkydri::Handle hd(w, h, n, {"tag36h11"}, 3, 1, 0);
                chalkydri::check(ck_upload_frames(hd.get(), imgs.data(), n), "ck_upload_frames");
                out = chalkydri::corner_subpix(hd, pp, fr, xy, &info);
            }
            std::ofstream o(argv[8], std::ios::binary);
            put(o, out);
            put(o, info);
            std::printf("OK %d\n", np);
            return 0;
        }
        if (cmd == "detect" && argc == 8) {
            chalkydri::Handle hd(w, h, n, {"tag36h11"}, 3, 1, 0);
            const int half = std::atoi(argv[5]);
            const ck_subpix_params_t pp = chalkydri::subpix_params(half);
            hd.set_corner_subpix(half ? &pp : nullptr);
            std::vector<ck_detection_t> dets((size_t)n * 64);
            std::memset(dets.data(), 0, dets.size() * sizeof(ck_detection_t));
            std::vector<int32_t> counts((size_t)n);
            chalkydri::check(ck_detect_batch(hd.get(), imgs.data(), n, dets.data(), 64, counts.data(), nullptr), "ck_detect_batch");
            std::ofstream o(argv[7], std::ios::binary);
            put(o, counts);
            put(o, dets);
            std::printf("OK %d\n", n);
            return 0;
        }
        if (board && argc == 9) {
            auto hd = std::make_shared<chalkydri::Handle>(w, h, n, std::vector<std::string>{"tag36h11"}, 3, 1, 0);
            chalkydri::Board b;
            b.rows = std::atoi(argv[5]); b.cols = std::atoi(argv[6]);
            std::vector<ck_detection_t> dets((size_t)n * 64);
            std::vector<int32_t> counts((size_t)n);
            chalkydri::check(ck_detect_batch(hd->get(), imgs.data(), n, dets.data(), 64, counts.data(), nullptr), "ck_detect_batch");
            const chalkydri::BoardCorners r = chalkydri::board_corners(*hd, b);
            std::ofstream o(argv[8], std::ios::binary);
            put(o, r.uv);
            put(o, r.state);
            put(o, r.n_tags);
            chalkydri::Calibrator rec(hd, b, 4, true), plain(hd, b, 4, false);
            const size_t fr = rec.process(imgs), fp = plain.process(imgs);
            std::printf("OK %d FRAMES %zu %zu\n", r.n_frames, fr, fp);
            return 0;
        }
        std::fprintf(stderr, "usage: see the head of tests/cpp/subpix_demo.cpp\n");
        return 2;
    } catch (const chalkydri::Panic &e) {
        std::fprintf(stderr, "panic: %s\n", e.what());
        return 3;
    }
}
