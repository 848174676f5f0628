// calib_demo — the C++ host layer's camera calibration (include/chalkydri.hpp: Board, Calibrator) driven from tests/test_cpp_calib.py
// and tests/test_gpu_calib.py.
//   calib_demo board ROWS COLS TAG_SIZE TAG_SPACING FIRST_ID OUT
//       OUT gets the corners of every tag, [rows * cols][4][2] doubles (no GPU needed)
//   calib_demo points W H MASK IN OUT
//       IN holds int32 F, int32 frame_start[F + 1], then board_xy and image_uv ([n][2] doubles each); the frames go through
//       Calibrator::add_observations and Calibrator::calibrate(MASK); OUT gets the ck_calib_result_t and the F poses behind it;
//       prints "OK" when calibrate returned a model, "NONE" otherwise
//   calib_demo frames W H MASK IN
//       IN holds int32 N, then N frames [H][W] of 8-bit luma: Calibrator::process, then calibrate; prints "KEPT k" and the model
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>

#include "chalkydri.hpp"

static std::vector<uint8_t> slurp(const char *path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

int main(int argc, char **argv) {
    try {
        const std::string cmd = argc > 1 ? argv[1] : "";
        if (cmd == "board" && argc == 8) {
            chalkydri::Board b;
            b.rows = std::atoi(argv[2]); b.cols = std::atoi(argv[3]);
            b.tag_size = std::atof(argv[4]); b.tag_spacing = std::atof(argv[5]);
            b.first_id = std::atoi(argv[6]);
            std::ofstream o(argv[7], std::ios::binary);
            for (int id = b.first_id; id < b.first_id + b.rows * b.cols; id++) {
                const auto c = b.tag_corners(id);
                o.write(reinterpret_cast<const char *>(c.data()), sizeof c);
            }
            (void)b.tag_corners(b.first_id + b.rows * b.cols); // a Panic: exit status 3
            return 0;
        }
        if ((cmd == "points" && argc == 7) || (cmd == "frames" && argc == 6)) {
            const int w = std::atoi(argv[2]), h = std::atoi(argv[3]);
            const uint32_t mask = (uint32_t)std::strtoul(argv[4], nullptr, 0);
            std::vector<uint8_t> in = slurp(argv[5]);
            if (in.size() < 4) { std::fprintf(stderr, "short input\n"); return 2; }
            int32_t n;
            std::memcpy(&n, in.data(), 4);
            auto handle = std::make_shared<chalkydri::Handle>(w, h, cmd == "frames" ? n : 1, std::vector<std::string>{"tag36h11"}, 3, 1, 0);
            chalkydri::Calibrator cal(handle);
            chalkydri::Calibrator::Report rep;
            if (cmd == "frames") {
                if (in.size() != 4 + (size_t)n * w * h) { std::fprintf(stderr, "not N frames\n"); return 2; }
                std::vector<ck_image_u8_t> imgs;
                for (int i = 0; i < n; i++) imgs.push_back({in.data() + 4 + (size_t)i * w * h, w, h, w});
                std::printf("KEPT %zu\n", cal.process(imgs));
            } else {
                std::vector<int32_t> starts(n + 1);
                if (in.size() < 4 + 4 * starts.size()) { std::fprintf(stderr, "short input\n"); return 2; }
                std::memcpy(starts.data(), in.data() + 4, 4 * starts.size());
                const size_t np = (size_t)starts[n], at = 4 + 4 * starts.size();
                if (in.size() != at + 32 * np) { std::fprintf(stderr, "not the points\n"); return 2; }
                std::vector<double> bxy(2 * np), uv(2 * np);
                std::memcpy(bxy.data(), in.data() + at, 16 * np);
                std::memcpy(uv.data(), in.data() + at + 16 * np, 16 * np);
                for (int f = 0; f < n; f++)
                    cal.add_observations(std::vector<double>(bxy.begin() + 2 * starts[f], bxy.begin() + 2 * starts[f + 1]),
                                         std::vector<double>(uv.begin() + 2 * starts[f], uv.begin() + 2 * starts[f + 1]));
            }
            const std::optional<chalkydri::OpenCv5> m = cal.calibrate(mask, &rep);
            if (cal.frames() != 0) { std::fprintf(stderr, "calibrate did not clear\n"); return 2; }
            if (cmd == "points") {
                std::ofstream o(argv[6], std::ios::binary);
                o.write(reinterpret_cast<const char *>(&rep.result), sizeof rep.result);
                o.write(reinterpret_cast<const char *>(rep.poses.data()), (std::streamsize)(rep.poses.size() * sizeof rep.poses[0]));
            }
            if (m) std::printf("OK %.17g %.17g %.17g %.17g rms %.6g\n", m->fx, m->fy, m->cx, m->cy, rep.result.rms);
            else std::printf("NONE %d\n", rep.result.status);
            return 0;
        }
        std::fprintf(stderr, "usage: calib_demo board|points|frames ...\n");
        return 2;
    } catch (const chalkydri::Panic &e) {
        std::fprintf(stderr, "panic: %s\n", e.what());
        return 3;
    }
}
