// exposure_demo — the C++ host layer's exposure entry points (include/chalkydri.hpp) driven from tests/test_cpp_exposure.py.
//   exposure_demo luts OUT                                 OUT = the 7 x 256 tables of the default parameters (no GPU needed)
//   exposure_demo recommend STATS EXPOSURE STEPS           STATS holds one ck_exposure_stats_t; prints the controller's exposure and
//                                                          gamma_hat after each of STEPS updates with it (no GPU needed)
//   exposure_demo roi W H MARGIN [X Y]...                  corners of detections, four per tag; prints "x0 y0 x1 y1" (no GPU needed)
//   exposure_demo stats W H N IN OUT [X0 Y0 X1 Y1]
//       IN holds N luma frames of W x H; OUT gets N records, record i of frame N-1-i (the index list is reversed), every frame
//       metered over the rectangle when one is given
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <iterator>

#include "chalkydri.hpp"

static std::vector<uint8_t> slurp(const char *path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
static void spill(const std::string &path, const void *p, size_t n) {
    std::ofstream(path, std::ios::binary).write(reinterpret_cast<const char *>(p), (std::streamsize)n);
}

int main(int argc, char **argv) {
    try {
        const std::string cmd = argc > 1 ? argv[1] : "";
        if (cmd == "luts" && argc >= 3) {
            const ck_exposure_params_t p = chalkydri::exposure_params();
            uint8_t lut[CK_EXPOSURE_GAMMAS * 256];
            chalkydri::check(ck_exposure_luts(&p, lut), "ck_exposure_luts");
            spill(argv[2], lut, sizeof lut);
            return 0;
        }
        if (cmd == "recommend" && argc >= 5) {
            const std::vector<uint8_t> b = slurp(argv[2]);
            if (b.size() != sizeof(ck_exposure_stats_t)) { std::fprintf(stderr, "not one record\n"); return 2; }
            ck_exposure_stats_t s;
            std::memcpy(&s, b.data(), sizeof s);
            chalkydri::ExposureController c(std::atof(argv[3]));
            for (int i = 0; i < std::atoi(argv[4]); i++) {
                const double e = c.update(s);
                std::printf("%.17g %.17g\n", e, c.gamma_hat());
            }
            return 0;
        }
        if (cmd == "roi" && argc >= 5 && (argc - 5) % 8 == 0) {
            std::vector<chalkydri::Detection> dets;
            for (int a = 5; a + 8 <= argc; a += 8) {
                ck_detection_t d{};
                for (int k = 0; k < 4; k++) { d.p[k][0] = std::atof(argv[a + 2 * k]); d.p[k][1] = std::atof(argv[a + 2 * k + 1]); }
                dets.emplace_back(d);
            }
            const ck_rect_t r = chalkydri::ExposureController::roi_from_detections(dets, std::atoi(argv[4]), std::atoi(argv[2]), std::atoi(argv[3]));
            std::printf("%d %d %d %d\n", r.x0, r.y0, r.x1, r.y1);
            return 0;
        }
        if (cmd == "stats" && (argc == 7 || argc == 11)) {
            const int w = std::atoi(argv[2]), h = std::atoi(argv[3]), n = std::atoi(argv[4]);
            std::vector<uint8_t> in = slurp(argv[5]);
            if (n < 1 || in.size() < (size_t)n * w * h) { std::fprintf(stderr, "input too short\n"); return 2; }
            std::vector<ck_image_u8_t> imgs;
            for (int i = 0; i < n; i++) imgs.push_back({in.data() + (size_t)i * w * h, w, h, w});
            chalkydri::Handle hd(w, h, n, {"tag36h11"}, 3, 1, 0);
            chalkydri::check(ck_upload_frames(hd.get(), imgs.data(), n), "ck_upload_frames");
            std::vector<int32_t> idx;
            for (int i = 0; i < n; i++) idx.push_back(n - 1 - i);
            std::vector<ck_rect_t> roi;
            if (argc == 11) roi.assign((size_t)n, ck_rect_t{std::atoi(argv[7]), std::atoi(argv[8]), std::atoi(argv[9]), std::atoi(argv[10])});
            const auto st = chalkydri::exposure_stats(hd, idx, chalkydri::exposure_params(), roi);
            spill(argv[6], st.data(), st.size() * sizeof(ck_exposure_stats_t));
            std::printf("OK %zu\n", st.size());
            return 0;
        }
        std::fprintf(stderr, "usage: exposure_demo luts|recommend|roi|stats ...\n");
        return 2;
    } catch (const chalkydri::Panic &e) {
        std::fprintf(stderr, "panic: %s\n", e.what());
        return 3;
    }
}
