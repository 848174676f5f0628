// jpeg_ring_demo — the C++ host layer's MJPEG entry points (include/chalkydri.hpp) driven from tests/test_cpp_jpeg_ring.py.
//   jpeg_ring_demo ORIENTATION W H N IN LUMA DETS
//       IN holds N JPEG frames, each behind its size as a little-endian int64; W x H is the ORIENTED frame.  The frames go
//       through a two-slot JPEG IngestRing (slot 1 first, then the same frames in reverse order through slot 0, both submitted
//       before either is processed).  LUMA gets the N oriented frames Handle::upload_jpeg stages, DETS the detections of slot 1
//       (int32 counts[N], then ck_detection_t[N][64]).  Prints "OK", then per frame "status/count/reversed/task": the frame's
//       CK_JPEG_* word from the ring, its detections, whether slot 0 found the same in frame N-1-i, and whether
//       AprilTags::process_jpeg with Config::{fourcc = MJPG, orientation} staged the same luma.
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
        if (argc < 8) {
            std::fprintf(stderr, "usage: jpeg_ring_demo ORIENTATION W H N IN LUMA DETS\n");
            return 2;
        }
        const int32_t o = chalkydri::orientation_code(argv[1]);
        const int w = std::atoi(argv[2]), h = std::atoi(argv[3]), n = std::atoi(argv[4]);
        const std::vector<uint8_t> in = slurp(argv[5]);
        std::vector<std::vector<uint8_t>> jpegs;
        size_t at = 0;
        for (int i = 0; i < n; i++) {
            int64_t size = 0;
            if (at + 8 > in.size()) { std::fprintf(stderr, "input too short\n"); return 2; }
            std::memcpy(&size, in.data() + at, 8);
            at += 8;
            if (size < 0 || at + (size_t)size > in.size()) { std::fprintf(stderr, "input too short\n"); return 2; }
            jpegs.emplace_back(in.begin() + (std::ptrdiff_t)at, in.begin() + (std::ptrdiff_t)(at + (size_t)size));
            at += (size_t)size;
        }
        if (n < 1) { std::fprintf(stderr, "no frames\n"); return 2; }
        auto hd = std::make_shared<chalkydri::Handle>(w, h, n, std::vector<std::string>{"tag36h11"}, 3, 1, 0);
        chalkydri::IngestRing ring(hd, 2, chalkydri::IngestRing::Jpeg{o, 0});
        for (int i = 0; i < n; i++) ring.write_jpeg(1, i, jpegs[(size_t)i]);
        ring.submit(1, n);
        for (int i = 0; i < n; i++) ring.write_jpeg(0, i, jpegs[(size_t)(n - 1 - i)]);
        ring.submit(0, n);
        std::vector<ck_detection_t> dets((size_t)n * 64), rev((size_t)n * 64);
        std::vector<int32_t> counts(n), rcounts(n);
        std::vector<uint32_t> st(n);
        chalkydri::check(ck_detect_ingested(ring.get(), 1, n, dets.data(), 64, counts.data(), st.data()), "ck_detect_ingested");
        chalkydri::check(ck_detect_ingested(ring.get(), 0, n, rev.data(), 64, rcounts.data(), st.data()), "ck_detect_ingested");
        const std::vector<uint32_t> jst = ring.jpeg_status(1, n);
        // the synchronous path stages the same luma ...
        const std::vector<uint8_t> luma = chalkydri::decode_jpeg(*hd, jpegs, o);
        std::ofstream(argv[6], std::ios::binary).write(reinterpret_cast<const char *>(luma.data()), (std::streamsize)luma.size());
        std::ofstream fd(argv[7], std::ios::binary);
        fd.write(reinterpret_cast<const char *>(counts.data()), (std::streamsize)(sizeof(int32_t) * counts.size()));
        fd.write(reinterpret_cast<const char *>(dets.data()), (std::streamsize)(sizeof(ck_detection_t) * dets.size()));
        // ... and so does the task with Config::{fourcc, orientation}
        chalkydri::AprilTags::Config c;
        c.width = (size_t)w; c.height = (size_t)h; c.max_batch = n;
        c.fourcc = "MJPG"; c.orientation = argv[1];
        c.calib.fx = c.calib.fy = 600.0; c.calib.cx = w / 2.0; c.calib.cy = h / 2.0;
        chalkydri::AprilTags task(c);
        (void)task.process_jpeg(jpegs, std::vector<std::optional<double>>((size_t)n, 0.0));
        std::vector<uint8_t> staged(luma.size());   // (quad_decimate 1, no filter: the quad image is the staged frame)
        chalkydri::check(ck_quad_image_batch(task.handle()->get(), nullptr, n, staged.data()), "ck_quad_image_batch");
        std::printf("OK");
        for (int i = 0; i < n; i++) {
            const int j = n - 1 - i;
            const bool same = counts[i] == rcounts[j] &&
                              std::memcmp(&dets[(size_t)i * 64], &rev[(size_t)j * 64], sizeof(ck_detection_t) * (size_t)std::min(counts[i], 64)) == 0;
            std::printf(" %u/%d/%d/%d", jst[(size_t)i], counts[i], (int)same, (int)(staged == luma));
        }
        std::printf("\n");
        return 0;
    } catch (const chalkydri::Panic &e) {
        std::printf("PANIC %s\n", e.what());
        return 3;
    }
}
