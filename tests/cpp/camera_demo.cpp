// camera_demo — the C++ host layer's camera models (include/chalkydri.hpp: Camera, Handle::set_camera, AprilTags::Config::camera,
// Calibrator::calibrate(CameraModel)) driven from tests/test_cpp_camera.py.
//   camera_demo model MODEL K0 .. K5 IN OUT
//       MODEL eucm | ucm (K5 ignored); IN holds pixels [n][2] doubles; OUT gets the bearings [n][3], the ok bytes [n] and the pixels
//       of Camera::project of those bearings [n][2] (no GPU needed); a camera that ck_camera_check refuses is a Panic: exit status 3
//   camera_demo points W H MODEL MASK IN OUT
//       IN holds int32 F, int32 frame_start[F + 1], then board_xy and image_uv ([n][2] doubles each); the frames go through
//       Calibrator::add_observations and Calibrator::calibrate(MODEL, MASK); OUT gets the ck_camera_calib_result_t and the F poses
//       behind it; prints "OK" and the model when calibrate returned one, "NONE" otherwise
//   camera_demo process W H F ALPHA BETA IN
//       IN holds one frame [H][W] of 8-bit luma: an AprilTags task with Config::camera = EUCM(F, F, W/2, H/2, ALPHA, BETA), a wall of
//       six tags as its layout, heading 0.05; prints "VALID v TAGS n" and the 64 bytes of the measurement in hex
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>

#include "chalkydri.hpp"

static std::vector<uint8_t> slurp(const char *path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static chalkydri::CameraModel model_of(const std::string &m) {
    if (m == "eucm") return chalkydri::CameraModel::Eucm;
    if (m == "ucm") return chalkydri::CameraModel::Ucm;
    if (m == "opencv5") return chalkydri::CameraModel::OpenCv5;
    throw chalkydri::Panic("unknown model", CK_EINVAL);
}

int main(int argc, char **argv) {
    try {
        const std::string cmd = argc > 1 ? argv[1] : "";
        if (cmd == "model" && argc == 11) {
            double k[6];
            for (int i = 0; i < 6; i++) k[i] = std::atof(argv[3 + i]);
            const chalkydri::Camera cam = model_of(argv[2]) == chalkydri::CameraModel::Ucm ? chalkydri::Camera::ucm(k[0], k[1], k[2], k[3], k[4])
                                                                                            : chalkydri::Camera::eucm(k[0], k[1], k[2], k[3], k[4], k[5]);
            const std::vector<uint8_t> in = slurp(argv[9]);
            std::vector<double> px(in.size() / 8);
            std::memcpy(px.data(), in.data(), px.size() * 8);
            std::vector<uint8_t> ok;
            const std::vector<double> b = cam.unproject(px, &ok), back = cam.project(b);
            std::ofstream o(argv[10], std::ios::binary);
            o.write(reinterpret_cast<const char *>(b.data()), (std::streamsize)(b.size() * 8));
            o.write(reinterpret_cast<const char *>(ok.data()), (std::streamsize)ok.size());
            o.write(reinterpret_cast<const char *>(back.data()), (std::streamsize)(back.size() * 8));
            std::printf("OK %zu\n", ok.size());
            return 0;
        }
        if (cmd == "points" && argc == 8) {
            const int w = std::atoi(argv[2]), h = std::atoi(argv[3]);
            const chalkydri::CameraModel model = model_of(argv[4]);
            const uint32_t mask = (uint32_t)std::strtoul(argv[5], nullptr, 0);
            const std::vector<uint8_t> in = slurp(argv[6]);
            if (in.size() < 4) { std::fprintf(stderr, "short input\n"); return 2; }
            int32_t n;
            std::memcpy(&n, in.data(), 4);
            std::vector<int32_t> starts(n + 1);
            if (in.size() < 4 + 4 * starts.size()) { std::fprintf(stderr, "short input\n"); return 2; }
            std::memcpy(starts.data(), in.data() + 4, 4 * starts.size());
            const size_t np = (size_t)starts[n], at = 4 + 4 * starts.size();
            if (in.size() != at + 32 * np) { std::fprintf(stderr, "not the points\n"); return 2; }
            std::vector<double> bxy(2 * np), uv(2 * np);
            std::memcpy(bxy.data(), in.data() + at, 16 * np);
            std::memcpy(uv.data(), in.data() + at + 16 * np, 16 * np);
            auto handle = std::make_shared<chalkydri::Handle>(w, h, 1, std::vector<std::string>{"tag36h11"}, 3, 1, 0);
            chalkydri::Calibrator cal(handle);
            for (int f = 0; f < n; f++)
                cal.add_observations(std::vector<double>(bxy.begin() + 2 * starts[f], bxy.begin() + 2 * starts[f + 1]),
                                     std::vector<double>(uv.begin() + 2 * starts[f], uv.begin() + 2 * starts[f + 1]));
            chalkydri::Calibrator::CameraReport rep;
            const std::optional<chalkydri::Camera> m = cal.calibrate(model, mask, &rep);
            if (cal.frames() != 0) { std::fprintf(stderr, "calibrate did not clear\n"); return 2; }
            std::ofstream o(argv[7], std::ios::binary);
            o.write(reinterpret_cast<const char *>(&rep.result), sizeof rep.result);
            o.write(reinterpret_cast<const char *>(rep.poses.data()), (std::streamsize)(rep.poses.size() * sizeof rep.poses[0]));
            if (m) std::printf("OK model %d start %d of %d rms %.6g\n", m->raw.model, rep.result.start, rep.result.n_starts, rep.result.rms);
            else std::printf("NONE %d\n", rep.result.status);
            return 0;
        }
        if (cmd == "process" && argc == 8) {
            const int w = std::atoi(argv[2]), h = std::atoi(argv[3]);
            const double f = std::atof(argv[4]);
            std::vector<uint8_t> in = slurp(argv[7]);
            if (in.size() != (size_t)w * h) { std::fprintf(stderr, "not one frame\n"); return 2; }
            chalkydri::AprilTags::Config c;
            c.width = (size_t)w; c.height = (size_t)h;
            c.calib = ck_opencv5_t{1, 1, 0, 0, 9, 9, 9, 9, 9}; // ignored: the camera below is set on the handle
            c.camera = chalkydri::Camera::eucm(f, f, w / 2.0, h / 2.0, std::atof(argv[5]), std::atof(argv[6]));
            c.robot_to_cam = {0, 0, 0, 0.2, 0.0, 0.6};
            c.cam_id = 3;
            for (int k = 0; k < 6; k++) // scenes.wall_layout(6, cols=3): x = 5, facing -x
                c.layout.emplace((size_t)(1 + k), chalkydri::sqpnp::Iso3{{5.0, (k % 3 - 1) * 0.45, 1.0 + (k / 3) * 0.45}, {6.123233995736766e-17, 0.0, 0.0, 1.0}});
            chalkydri::AprilTags task(c);
            const std::vector<ck_image_u8_t> imgs{ck_image_u8_t{in.data(), w, h, w}};
            const std::vector<std::optional<double>> gyro{0.05};
            const auto out = task.process(imgs, gyro);
            std::printf("VALID %d TAGS %d ", out[0].second ? 1 : 0, (int)out[0].first.tag_count);
            const ck_vision_measurement_t m = out[0].first;
            for (size_t i = 0; i < sizeof m; i++) std::printf("%02x", reinterpret_cast<const uint8_t *>(&m)[i]);
            std::printf("\n");
            return 0;
        }
        std::fprintf(stderr, "usage: camera_demo model|points|process ...\n");
        return 2;
    } catch (const chalkydri::Panic &e) {
        std::fprintf(stderr, "panic: %s\n", e.what());
        return 3;
    }
}
