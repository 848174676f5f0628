// rig_demo — the C++ host layer of the camera rig (include/chalkydri.hpp: RigSolver), driven from tests/test_cpp_rig.py.
//   rig_demo host  IN OUT   RigSolver::solve_host on the steps of IN (no device), the result records to OUT
//   rig_demo batch IN OUT   RigSolver::solve_batch on a handle of its own
//   rig_demo last  IN OUT   two AprilTags tasks process their frames, then chalkydri::rig_process_last (rig_id 42): the measurements,
//                           the valid flags (int32) and the result records to OUT.  IN: int32 n, per camera (two) int32 w, h, double f,
//                           x, y, z, roll, pitch, yaw of the mount and n frames of w * h bytes, then n gyro headings and n int32
//                           "has a heading"; the field is the wall of 12 tags of chalkydri_amd/scenes.py (wall_layout)
// IN: int32 n, int32 n_cams, then per step and camera int32 n_tags, robot_to_cam [7], n_tags tags [7], 4 * n_tags bearings [3]; then
// n gyro headings.  Isometries are t[3], q[4] (w, x, y, z).
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <map>
#include <memory>
#include <optional>
#include <string>
#include <vector>

#include "chalkydri.hpp"

using namespace chalkydri;

struct Reader {
    std::vector<char> buf;
    size_t at = 0;
    template <typename T>
    T get() {
        T v;
        if (at + sizeof v > buf.size()) throw Panic("rig_demo: input too short");
        std::memcpy(&v, buf.data() + at, sizeof v);
        at += sizeof v;
        return v;
    }
    sqpnp::Iso3 iso() {
        ck_iso3_t r;
        for (double &v : r.t) v = get<double>();
        for (double &v : r.q) v = get<double>();
        return sqpnp::Iso3::from_raw(r);
    }
};

static int last(Reader &rd, const char *out_path) {
    const int n = rd.get<int32_t>();
    std::map<size_t, sqpnp::Iso3> layout;
    for (int k = 0; k < 12; k++) {
        sqpnp::Iso3 t;
        t.translation = {5.0, (k % 6 - 2.5) * 0.45, 1.0 + (k / 6) * 0.45};
        t.rotation = {6.123233995736766e-17, 0.0, 0.0, 1.0};
        layout[(size_t)(k + 1)] = t;
    }
    std::vector<std::unique_ptr<AprilTags>> tasks;
    std::vector<std::vector<uint8_t>> pixels(2);
    std::vector<std::vector<ck_image_u8_t>> imgs(2);
    for (int c = 0; c < 2; c++) {
        AprilTags::Config cfg;
        cfg.width = (size_t)rd.get<int32_t>(); cfg.height = (size_t)rd.get<int32_t>();
        const double f = rd.get<double>();
        cfg.calib = ck_opencv5_t{f, f, cfg.width / 2.0, cfg.height / 2.0, 0, 0, 0, 0, 0};
        cfg.robot_to_cam.x = rd.get<double>(); cfg.robot_to_cam.y = rd.get<double>(); cfg.robot_to_cam.z = rd.get<double>();
        cfg.robot_to_cam.roll = rd.get<double>(); cfg.robot_to_cam.pitch = rd.get<double>(); cfg.robot_to_cam.yaw = rd.get<double>();
        cfg.layout = layout; cfg.cam_id = (uint8_t)c; cfg.max_batch = n;
        const size_t bytes = cfg.width * cfg.height;
        pixels[c].resize(bytes * (size_t)n);
        for (auto &b : pixels[c]) b = rd.get<uint8_t>();
        for (int i = 0; i < n; i++) imgs[c].push_back(ck_image_u8_t{pixels[c].data() + bytes * (size_t)i, (int32_t)cfg.width, (int32_t)cfg.height, (int32_t)cfg.width});
        tasks.push_back(std::make_unique<AprilTags>(cfg));
    }
    std::vector<double> g(n);
    for (double &v : g) v = rd.get<double>();
    std::vector<std::optional<double>> gyro;
    for (int i = 0; i < n; i++) gyro.push_back(rd.get<int32_t>() ? std::optional<double>(g[i]) : std::nullopt);
    for (int c = 0; c < 2; c++) (void)tasks[c]->process(imgs[c], gyro);
    std::vector<ck_rig_result_t> res;
    const auto recs = rig_process_last({tasks[0].get(), tasks[1].get()}, RigSolver().rig_id(42).params(), gyro, &res);
    std::ofstream out(out_path, std::ios::binary);
    int valid = 0;
    for (const auto &r : recs) out.write(reinterpret_cast<const char *>(&r.first), sizeof r.first);
    for (const auto &r : recs) { const int32_t v = r.second; valid += v; out.write(reinterpret_cast<const char *>(&v), sizeof v); }
    out.write(reinterpret_cast<const char *>(res.data()), (std::streamsize)(res.size() * sizeof(ck_rig_result_t)));
    std::printf("OK %d of %d\n", valid, n);
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 4) { std::fprintf(stderr, "usage: rig_demo host|batch|last IN OUT\n"); return 2; }
    try {
        const std::string mode = argv[1];
        std::ifstream in(argv[2], std::ios::binary);
        Reader rd{std::vector<char>(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>())};
        if (mode == "last") return last(rd, argv[3]);
        const int n = rd.get<int32_t>(), n_cams = rd.get<int32_t>();
        std::vector<std::vector<RigView>> steps(n, std::vector<RigView>(n_cams));
        for (auto &step : steps)
            for (auto &v : step) {
                const int nt = rd.get<int32_t>();
                v.robot_to_cam = rd.iso();
                for (int t = 0; t < nt; t++) v.tags.push_back(rd.iso());
                for (int b = 0; b < 4 * nt; b++) { sqpnp::Vec3 x; for (double &e : x) e = rd.get<double>(); v.bearings.push_back(x); }
            }
        std::vector<double> gyro(n);
        for (double &g : gyro) g = rd.get<double>();
        std::vector<ck_rig_result_t> res;
        if (mode == "host") res = RigSolver().solve_host(steps, gyro);
        else if (mode == "batch") res = RigSolver(std::make_shared<Handle>(64, 64, 1, std::vector<std::string>{"tag36h11"}, 3, 1, 0)).solve_batch(steps, gyro);
        else throw Panic("rig_demo: unknown mode " + mode);
        std::ofstream out(argv[3], std::ios::binary);
        out.write(reinterpret_cast<const char *>(res.data()), (std::streamsize)(res.size() * sizeof(ck_rig_result_t)));
        int valid = 0;
        for (const auto &r : res) valid += r.valid;
        std::printf("OK %d of %d\n", valid, n);
        return 0;
    } catch (const Panic &p) {
        std::fprintf(stderr, "panic: %s\n", p.what());
        return 3;
    }
}
