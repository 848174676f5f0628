// rigcal_demo — the C++ host layer's MountCalibrator (include/chalkydri.hpp) on a capture written by tests/test_cpp_rigcal.py:
//   rigcal_demo host|batch|calibrate IN OUT
// IN: int32 n_cams, n_steps, max_iters; uint64 fixed_mask; mounts0 [n_cams][7] (t, q); per step: gyro, poses0 [12], per camera int32
// n_tags, tags [n_tags][7], bearings [n_tags][12].  host: ck_rigcal_refine_host without a device; batch: ck_rigcal_refine_batch on a
// handle of its own; calibrate: ck_rig_calibrate_batch.  OUT: the result record, then the poses [n_steps][12].  Prints OK or NONE.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "chalkydri.hpp"

namespace {
struct Reader {
    std::vector<uint8_t> d;
    size_t at = 0;
    template <typename T>
    T get() {
        T v;
        if (at + sizeof v > d.size()) throw chalkydri::Panic("input too short", CK_EINVAL);
        std::memcpy(&v, d.data() + at, sizeof v);
        at += sizeof v;
        return v;
    }
};
} // namespace

int main(int argc, char **argv) {
    try {
        if (argc < 4) throw chalkydri::Panic("usage: rigcal_demo host|batch|calibrate IN OUT", CK_EINVAL);
        const std::string cmd = argv[1];
        std::ifstream f(argv[2], std::ios::binary);
        Reader in;
        in.d.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
        const int C = in.get<int32_t>(), n = in.get<int32_t>(), max_iters = in.get<int32_t>();
        in.get<int32_t>();
        const uint64_t mask = in.get<uint64_t>();
        std::vector<ck_iso3_t> mounts0((size_t)C);
        for (auto &m : mounts0) m = in.get<ck_iso3_t>();
        std::shared_ptr<chalkydri::Handle> handle;
        if (cmd != "host") handle = std::make_shared<chalkydri::Handle>(64, 64, 1, std::vector<std::string>{"tag36h11"}, 3, 1, 0);
        chalkydri::MountCalibrator mc(handle, mounts0, mask);
        std::vector<std::array<double, 12>> poses0((size_t)n);
        for (int s = 0; s < n; s++) {
            const double gyro = in.get<double>();
            poses0[(size_t)s] = in.get<std::array<double, 12>>();
            std::vector<std::vector<ck_iso3_t>> tags((size_t)C);
            std::vector<std::vector<double>> bear((size_t)C);
            for (int c = 0; c < C; c++) {
                const int nt = in.get<int32_t>();
                for (int k = 0; k < nt; k++) tags[(size_t)c].push_back(in.get<ck_iso3_t>());
                for (int k = 0; k < 12 * nt; k++) bear[(size_t)c].push_back(in.get<double>());
            }
            mc.add_step(tags, bear, gyro);
        }
        if ((int)mc.steps() != n) throw chalkydri::Panic("steps", CK_EINVAL);
        chalkydri::MountCalibrator::Report rep;
        const auto got = cmd == "calibrate" ? mc.calibrate(&rep, max_iters) : mc.refine(poses0, cmd == "host", &rep, max_iters);
        std::ofstream o(argv[3], std::ios::binary);
        o.write(reinterpret_cast<const char *>(&rep.result), sizeof rep.result);
        for (const auto &P : rep.poses) o.write(reinterpret_cast<const char *>(P.data()), sizeof(double) * 12);
        std::printf("%s %d iterations, status %d\n", got ? "OK" : "NONE", rep.result.iters, rep.result.status);
        mc.clear();
        return mc.steps() == 0 ? 0 : 1;
    } catch (const chalkydri::Panic &e) {
        std::fprintf(stderr, "panic: %s\n", e.what());
        return 3;
    }
}
