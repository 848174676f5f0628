// tri_otsu_demo — the C++ host layer's tri-class threshold (include/chalkydri.hpp) driven from tests/test_cpp_tri_otsu.py.
//   tri_otsu_demo solve HIST OUT [MAX_ITERS MIN_DELTA KEEP_TBD]
//       HIST holds 256 uint32 counts; OUT gets the ck_tri_otsu_info_t and the 256-byte table behind it (no GPU needed)
//   tri_otsu_demo frame W H CHANNELS KEEP_TBD IN OUT
//       IN holds one frame [H][W][CHANNELS]; OUT gets the record and the class map behind it; prints "OK <corners>" after
//       Detector::tri_otsu and Detector::detect_corners on the detector's class map
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

int main(int argc, char **argv) {
    try {
        const std::string cmd = argc > 1 ? argv[1] : "";
        if (cmd == "solve" && (argc == 4 || argc == 7)) {
            const std::vector<uint8_t> b = slurp(argv[2]);
            std::array<uint32_t, 256> hist;
            if (b.size() != sizeof hist) { std::fprintf(stderr, "not 256 counts\n"); return 2; }
            std::memcpy(hist.data(), b.data(), sizeof hist);
            ck_tri_otsu_params_t p = chalkydri::tri_otsu_params();
            if (argc == 7) { p.max_iters = std::atoi(argv[4]); p.min_delta = std::atoi(argv[5]); p.keep_tbd = std::atoi(argv[6]); }
            const chalkydri::TriOtsu r = chalkydri::tri_otsu_solve(hist, p);
            std::ofstream o(argv[3], std::ios::binary);
            o.write(reinterpret_cast<const char *>(&r.info), sizeof r.info);
            o.write(reinterpret_cast<const char *>(r.lut.data()), (std::streamsize)r.lut.size());
            return 0;
        }
        if (cmd == "frame" && argc == 8) {
            const int w = std::atoi(argv[2]), h = std::atoi(argv[3]);
            ck_tri_otsu_params_t p = chalkydri::tri_otsu_params();
            p.channels = std::atoi(argv[4]); p.keep_tbd = std::atoi(argv[5]);
            const std::vector<uint8_t> in = slurp(argv[6]);
            chalkydri::apriltags::Detector det((size_t)w, (size_t)h, {});
            const ck_tri_otsu_info_t info = det.tri_otsu(in, p);
            det.detect_corners();
            std::ofstream o(argv[7], std::ios::binary);
            o.write(reinterpret_cast<const char *>(&info), sizeof info);
            o.write(reinterpret_cast<const char *>(det.buf().data()), (std::streamsize)det.buf().size());
            std::printf("OK %zu\n", det.points().size());
            return 0;
        }
        std::fprintf(stderr, "usage: tri_otsu_demo solve|frame ...\n");
        return 2;
    } catch (const chalkydri::Panic &e) {
        std::fprintf(stderr, "panic: %s\n", e.what());
        return 3;
    }
}
