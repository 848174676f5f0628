// raw_demo — the C++ host layer's raw-format entry points (include/chalkydri.hpp) driven from tests/test_cpp_raw.py.
//   raw_demo layout FOURCC ORIENTATION W H            prints "sw sh min_stride min_bytes" (no GPU needed)
//   raw_demo luma FOURCC ORIENTATION W H N STRIDE IN OUT
//       IN holds N source frames of sh rows x STRIDE bytes; OUT gets the N oriented W x H luma frames the device stages,
//       then prints per frame "detections/1": the tags ck_detect_uploaded finds behind Handle::upload_raw, and whether
//       AprilTags::process with Config::{fourcc, orientation} staged the same luma
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
        if (argc >= 6 && std::string(argv[1]) == "layout") {
            const chalkydri::RawLayout l = chalkydri::raw_layout(chalkydri::raw_format(argv[2], argv[3]), std::atoi(argv[4]), std::atoi(argv[5]));
            std::printf("%d %d %d %lld\n", l.sw, l.sh, l.min_stride, (long long)l.min_bytes);
            return 0;
        }
        if (argc >= 10 && std::string(argv[1]) == "luma") {
            const ck_raw_format_t fmt = chalkydri::raw_format(argv[2], argv[3]);
            const int w = std::atoi(argv[4]), h = std::atoi(argv[5]), n = std::atoi(argv[6]), stride = std::atoi(argv[7]);
            const chalkydri::RawLayout l = chalkydri::raw_layout(fmt, w, h);
            std::vector<uint8_t> in = slurp(argv[8]);
            if (n < 1 || in.size() < (size_t)n * l.sh * stride) { std::fprintf(stderr, "input too short\n"); return 2; }
            std::vector<ck_image_u8_t> imgs;
            for (int i = 0; i < n; i++) imgs.push_back({in.data() + (size_t)i * l.sh * stride, l.sw, l.sh, stride});
            chalkydri::Handle hd(w, h, n, {"tag36h11"}, 3, 1, 0);
            const std::vector<uint8_t> luma = hd.raw_luma(imgs, fmt);
            std::ofstream(argv[9], std::ios::binary).write(reinterpret_cast<const char *>(luma.data()), (std::streamsize)luma.size());
            // the staged frames feed the detector as after ck_upload_frames
            std::vector<ck_detection_t> dets((size_t)n * 64);
            std::vector<int32_t> counts(n);
            std::vector<uint32_t> st(n);
            hd.upload_raw(imgs, fmt);
            chalkydri::check(ck_detect_uploaded(hd.get(), n, dets.data(), 64, counts.data(), st.data()), "ck_detect_uploaded");
            // and the task with Config::{fourcc, orientation} takes the camera's frames as they are
            chalkydri::AprilTags::Config c;
            c.width = (size_t)w; c.height = (size_t)h; c.max_batch = n;
            c.fourcc = argv[2]; c.orientation = argv[3];
            c.calib.fx = c.calib.fy = 600.0; c.calib.cx = w / 2.0; c.calib.cy = h / 2.0;
            chalkydri::AprilTags task(c);
            (void)task.process(imgs, std::vector<std::optional<double>>((size_t)n, 0.0));
            std::vector<uint8_t> staged(luma.size());   // (quad_decimate 1, no filter: the quad image is the staged frame)
            chalkydri::check(ck_quad_image_batch(task.handle()->get(), nullptr, n, staged.data()), "ck_quad_image_batch");
            std::printf("OK");
            for (int i = 0; i < n; i++) std::printf(" %d/%d", counts[i], (int)(staged == luma));
            std::printf("\n");
            return 0;
        }
        std::fprintf(stderr, "usage: raw_demo layout FOURCC ORIENTATION W H | raw_demo luma FOURCC ORIENTATION W H N STRIDE IN OUT\n");
        return 2;
    } catch (const chalkydri::Panic &e) {
        std::printf("PANIC %s\n", e.what());
        return 3;
    }
}
