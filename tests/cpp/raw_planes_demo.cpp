// raw_planes_demo — the C++ host layer on the planar 4:2:0 raw formats with their chroma planes (include/chalkydri.hpp: raw_format's
// `planes`, raw_plane_layout), driven from tests/test_cpp_raw_planes.py.
//   raw_planes_demo layout FOURCC ORIENTATION W H STRIDE
//       prints "sw sh cw ch  off0 off1 off2  rs0 rs1 rs2  st0 st1 st2  bytes" of the source of an oriented W x H frame (no device)
//   raw_planes_demo color FOURCC ORIENTATION W H STRIDE QUALITY N IN OUT_PREFIX
//       IN holds N frames of FOURCC with their planes at row stride STRIDE; OUT_PREFIX<i>.jpg gets the colour preview of frame i at
//       the frame's own size, from the handle's raw staging
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>

#include "chalkydri.hpp"

int main(int argc, char **argv) {
    try {
        if (argc < 7 || std::strlen(argv[2]) != 4) { std::fprintf(stderr, "usage: raw_planes_demo layout|color FOURCC ORIENTATION W H STRIDE ...\n"); return 2; }
        const std::string form = argv[1];
        const ck_raw_format_t fmt = chalkydri::raw_format(argv[2], argv[3], true);
        const int w = std::atoi(argv[4]), h = std::atoi(argv[5]), stride = std::atoi(argv[6]);
        const ck_raw_planes_t p = chalkydri::raw_plane_layout(fmt, w, h, stride);
        if (form == "layout") {
            std::printf("%d %d %d %d  %lld %lld %lld  %d %d %d  %d %d %d  %lld\n", p.sw, p.sh, p.cw, p.ch, (long long)p.offset[0], (long long)p.offset[1],
                        (long long)p.offset[2], p.row_stride[0], p.row_stride[1], p.row_stride[2], p.step[0], p.step[1], p.step[2], (long long)p.bytes);
            return 0;
        }
        if (form != "color" || argc < 11) { std::fprintf(stderr, "usage: raw_planes_demo color FOURCC ORIENTATION W H STRIDE QUALITY N IN OUT_PREFIX\n"); return 2; }
        const int n = std::atoi(argv[8]);
        std::ifstream f(argv[9], std::ios::binary);
        std::vector<uint8_t> in((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        if (n < 1 || in.size() < (size_t)n * (size_t)p.bytes) { std::fprintf(stderr, "input too short\n"); return 2; }
        std::vector<ck_image_u8_t> imgs;
        for (int i = 0; i < n; i++) imgs.push_back({in.data() + (size_t)i * (size_t)p.bytes, p.sw, p.sh, stride});
        auto hd = std::make_shared<chalkydri::Handle>(w, h, n, std::vector<std::string>{"tag36h11"}, 3, 1, 0);
        hd->upload_raw(imgs, fmt);
        std::vector<int32_t> idx;
        for (int i = 0; i < n; i++) idx.push_back(i);
        const auto files = chalkydri::preview_jpeg_color(*hd, idx, chalkydri::preview_params(0, 0, std::atoi(argv[7]), 0));
        for (int i = 0; i < n; i++)
            std::ofstream(std::string(argv[10]) + std::to_string(i) + ".jpg", std::ios::binary)
                .write(reinterpret_cast<const char *>(files[i].data()), (std::streamsize)files[i].size());
        std::printf("OK %zu\n", files.size());
        return 0;
    } catch (const chalkydri::Panic &e) {
        std::fprintf(stderr, "panic: %s\n", e.what());
        return 3;
    }
}
