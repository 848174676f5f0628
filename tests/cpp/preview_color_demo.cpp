// preview_color_demo — the C++ host layer's colour preview (include/chalkydri.hpp: preview_jpeg_color, IngestRing::preview_jpeg_color)
// driven from tests/test_cpp_preview_color.py.
//   preview_color_demo host|ring FOURCC ORIENTATION WIDTH HEIGHT QUALITY RESTART_ROWS W H N IN OUT_PREFIX
//       IN holds N raw frames of FOURCC at their minimum stride, the sources of an oriented W x H frame; OUT_PREFIX<i>.jpg gets the
//       colour preview of frame N-1-i (the index list is reversed), from the handle's raw staging or from slot 1 of a raw ring
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>
#include <memory>

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
        if (argc < 13 || std::strlen(argv[2]) != 4) { std::fprintf(stderr, "usage: preview_color_demo host|ring FOURCC ...\n"); return 2; }
        const std::string form = argv[1];
        const char *c = argv[2];
        const ck_raw_format_t fmt = {(uint32_t)(uint8_t)c[0] | ((uint32_t)(uint8_t)c[1] << 8) | ((uint32_t)(uint8_t)c[2] << 16) | ((uint32_t)(uint8_t)c[3] << 24),
                                     std::atoi(argv[3])};
        const ck_preview_params_t pp = chalkydri::preview_params(std::atoi(argv[4]), std::atoi(argv[5]), std::atoi(argv[6]), std::atoi(argv[7]));
        const int w = std::atoi(argv[8]), h = std::atoi(argv[9]), n = std::atoi(argv[10]);
        int32_t sw = 0, sh = 0, stride = 0;
        int64_t bytes = 0;
        chalkydri::check(ck_raw_layout(&fmt, w, h, &sw, &sh, &stride, &bytes), "ck_raw_layout");
        std::vector<uint8_t> in = slurp(argv[11]);
        if (n < 1 || in.size() < (size_t)n * (size_t)bytes) { std::fprintf(stderr, "input too short\n"); return 2; }
        std::vector<ck_image_u8_t> imgs;
        for (int i = 0; i < n; i++) imgs.push_back({in.data() + (size_t)i * (size_t)bytes, sw, sh, stride});
        auto hd = std::make_shared<chalkydri::Handle>(w, h, n, std::vector<std::string>{"tag36h11"}, 3, 1, 0);
        std::vector<int32_t> idx;
        for (int i = 0; i < n; i++) idx.push_back(n - 1 - i);
        std::vector<std::vector<uint8_t>> files;
        if (form == "ring") {
            chalkydri::IngestRing ring(hd, 2, fmt);
            for (int i = 0; i < n; i++) ring.write(1, i, imgs[i], fmt.fourcc);
            ring.submit(1, n);
            files = ring.preview_jpeg_color(1, idx, pp);
        } else {
            chalkydri::check(ck_upload_raw(hd->get(), imgs.data(), n, &fmt), "ck_upload_raw");
            files = chalkydri::preview_jpeg_color(*hd, idx, pp);
        }
        for (int i = 0; i < n; i++) spill(std::string(argv[12]) + std::to_string(i) + ".jpg", files[i]);
        std::printf("OK %zu\n", files.size());
        return 0;
    } catch (const chalkydri::Panic &e) {
        std::fprintf(stderr, "panic: %s\n", e.what());
        return 3;
    }
}
