// blobs_demo — the C++ host layer's coloured-piece detector (include/chalkydri.hpp: BlobParams, detect_blobs, Handle::detect_blobs)
// driven from tests/test_gpu_blobs.py.
//   blobs_demo FOURCC ORIENTATION W H N H_MIN H_MAX S_MIN V_MIN MIN_AREA IN OUT
//       IN holds N raw frames of FOURCC at their minimum stride, the sources of an oriented W x H frame; OUT gets the records
//       [N][1][16] of frame N-1-i (the index list is reversed), then the counts [N] and the status [N]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>

#include "chalkydri.hpp"

static std::vector<uint8_t> slurp(const char *path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

int main(int argc, char **argv) {
    try {
        if (argc < 13 || std::strlen(argv[1]) != 4) { std::fprintf(stderr, "usage: blobs_demo FOURCC ORIENTATION W H N H_MIN H_MAX S_MIN V_MIN MIN_AREA IN OUT\n"); return 2; }
        const char *c = argv[1];
        const ck_raw_format_t fmt = {(uint32_t)(uint8_t)c[0] | ((uint32_t)(uint8_t)c[1] << 8) | ((uint32_t)(uint8_t)c[2] << 16) | ((uint32_t)(uint8_t)c[3] << 24),
                                     std::atoi(argv[2])};
        const int w = std::atoi(argv[3]), h = std::atoi(argv[4]), n = std::atoi(argv[5]);
        chalkydri::BlobParams pp;
        pp.hsv(0, std::atoi(argv[6]), std::atoi(argv[7]), std::atoi(argv[8]), 255, std::atoi(argv[9]), 255);
        pp.cls(0).min_area = std::atoi(argv[10]);
        pp.check_ok();
        int32_t sw = 0, sh = 0, stride = 0;
        int64_t bytes = 0;
        chalkydri::check(ck_raw_layout(&fmt, w, h, &sw, &sh, &stride, &bytes), "ck_raw_layout");
        std::vector<uint8_t> in = slurp(argv[11]);
        if (n < 1 || in.size() < (size_t)n * (size_t)bytes) { std::fprintf(stderr, "input too short\n"); return 2; }
        std::vector<ck_image_u8_t> imgs;
        for (int i = 0; i < n; i++) imgs.push_back({in.data() + (size_t)i * (size_t)bytes, sw, sh, stride});
        chalkydri::Handle hd(w, h, n, std::vector<std::string>{"tag36h11"}, 3, 1, 0);
        hd.upload_raw(imgs, fmt);
        std::vector<int32_t> idx;
        for (int i = 0; i < n; i++) idx.push_back(n - 1 - i);
        const auto r = chalkydri::detect_blobs(hd, pp, idx);
        std::ofstream out(argv[12], std::ios::binary);
        out.write(reinterpret_cast<const char *>(r.records.data()), (std::streamsize)(r.records.size() * sizeof(ck_blob_t)));
        out.write(reinterpret_cast<const char *>(r.counts.data()), (std::streamsize)(r.counts.size() * sizeof(int32_t)));
        out.write(reinterpret_cast<const char *>(r.status.data()), (std::streamsize)(r.status.size() * sizeof(uint32_t)));
        std::printf("OK %zu %d\n", r.records.size(), r.cap);
        return 0;
    } catch (const chalkydri::Panic &e) {
        std::fprintf(stderr, "panic: %s\n", e.what());
        return 3;
    }
}
