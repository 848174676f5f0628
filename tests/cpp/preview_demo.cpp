// preview_demo — the C++ host layer's preview entry points (include/chalkydri.hpp) driven from tests/test_cpp_preview.py.
//   preview_demo layout WIDTH HEIGHT QUALITY RESTART_ROWS W H      prints "pw ph max_bytes" (no GPU needed)
//   preview_demo part IN OUT                                       OUT = mjpeg_part(IN) (no GPU needed)
//   preview_demo jpeg WIDTH HEIGHT QUALITY RESTART_ROWS W H N IN OUT_PREFIX
//       IN holds N luma frames of W x H; OUT_PREFIX<i>.jpg gets the preview of frame N-1-i (the index list is reversed)
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
static void spill(const std::string &path, const std::vector<uint8_t> &b) {
    std::ofstream(path, std::ios::binary).write(reinterpret_cast<const char *>(b.data()), (std::streamsize)b.size());
}

int main(int argc, char **argv) {
    try {
        const std::string cmd = argc > 1 ? argv[1] : "";
        if (cmd == "part" && argc >= 4) {
            spill(argv[3], chalkydri::mjpeg_part(slurp(argv[2])));
            return 0;
        }
        if ((cmd == "layout" && argc >= 8) || (cmd == "jpeg" && argc >= 11)) {
            const ck_preview_params_t pp = chalkydri::preview_params(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]));
            const int w = std::atoi(argv[6]), h = std::atoi(argv[7]);
            if (cmd == "layout") {
                int32_t pw = 0, ph = 0;
                int64_t mb = 0;
                chalkydri::check(ck_preview_layout(&pp, w, h, &pw, &ph, &mb), "ck_preview_layout");
                std::printf("%d %d %lld\n", pw, ph, (long long)mb);
                return 0;
            }
            const int n = std::atoi(argv[8]);
            std::vector<uint8_t> in = slurp(argv[9]);
            if (n < 1 || in.size() < (size_t)n * w * h) { std::fprintf(stderr, "input too short\n"); return 2; }
            std::vector<ck_image_u8_t> imgs;
            for (int i = 0; i < n; i++) imgs.push_back({in.data() + (size_t)i * w * h, w, h, w});
            chalkydri::Handle hd(w, h, n, {"tag36h11"}, 3, 1, 0);
            chalkydri::check(ck_upload_frames(hd.get(), imgs.data(), n), "ck_upload_frames");
            std::vector<int32_t> idx;
            for (int i = 0; i < n; i++) idx.push_back(n - 1 - i);
            const auto files = chalkydri::preview_jpeg(hd, idx, pp);
            for (int i = 0; i < n; i++) spill(std::string(argv[10]) + std::to_string(i) + ".jpg", files[i]);
            std::printf("OK %zu\n", files.size());
            return 0;
        }
        std::fprintf(stderr, "usage: preview_demo layout|part|jpeg ...\n");
        return 2;
    } catch (const chalkydri::Panic &e) {
        std::fprintf(stderr, "panic: %s\n", e.what());
        return 3;
    }
}
