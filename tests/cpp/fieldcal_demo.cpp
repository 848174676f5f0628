// fieldcal_demo — the C++ host layer's FieldCalibrator (include/chalkydri.hpp) on a capture written by tests/test_cpp_fieldcal.py:
//   fieldcal_demo host|batch|calibrate IN OUT
// IN: int32 n_cams, n_steps, n_layout, max_iters; mounts [n_cams][7] (t, q); layout [n_layout][7]; masks [n_layout] bytes; per step:
// gyro, poses0 [12], per camera int32 n_tags, layout entries [n_tags] int32, bearings [n_tags][12].  host: ck_fieldcal_refine_host
// without a device; batch: ck_fieldcal_refine_batch on a handle of its own; calibrate: ck_field_calibrate_batch.  OUT: the result
// record, the layout, the sightings, the tags' rms, then the poses [n_steps][12].  Prints OK or NONE.
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
        if (argc < 4) throw chalkydri::Panic("usage: fieldcal_demo host|batch|calibrate IN OUT", CK_EINVAL);
        const std::string cmd = argv[1];
        std::ifstream f(argv[2], std::ios::binary);
        Reader in;
        in.d.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
        const int C = in.get<int32_t>(), n = in.get<int32_t>(), L = in.get<int32_t>(), max_iters = in.get<int32_t>();
        std::vector<ck_iso3_t> mounts((size_t)C), layout((size_t)L);
        std::vector<uint8_t> masks((size_t)L);
        for (auto &m : mounts) m = in.get<ck_iso3_t>();
        for (auto &t : layout) t = in.get<ck_iso3_t>();
        for (auto &m : masks) m = in.get<uint8_t>();
        std::shared_ptr<chalkydri::Handle> handle;
        if (cmd != "host") handle = std::make_shared<chalkydri::Handle>(64, 64, 1, std::vector<std::string>{"tag36h11"}, 3, 1, 0);
        chalkydri::FieldCalibrator fc(handle, mounts, layout, masks);
        std::vector<std::array<double, 12>> poses0((size_t)n);
        for (int s = 0; s < n; s++) {
            const double gyro = in.get<double>();
            poses0[(size_t)s] = in.get<std::array<double, 12>>();
            std::vector<std::vector<int32_t>> tags((size_t)C);
            std::vector<std::vector<double>> bear((size_t)C);
            for (int c = 0; c < C; c++) {
                const int nt = in.get<int32_t>();
                for (int k = 0; k < nt; k++) tags[(size_t)c].push_back(in.get<int32_t>());
                for (int k = 0; k < 12 * nt; k++) bear[(size_t)c].push_back(in.get<double>());
            }
            fc.add_step(tags, bear, gyro);
        }
        if ((int)fc.steps() != n) throw chalkydri::Panic("steps", CK_EINVAL);
        chalkydri::FieldCalibrator::Report rep;
        const auto got = cmd == "calibrate" ? fc.calibrate(&rep, max_iters) : fc.refine(poses0, cmd == "host", &rep, max_iters);
        std::ofstream o(argv[3], std::ios::binary);
        o.write(reinterpret_cast<const char *>(&rep.result), sizeof rep.result);
        o.write(reinterpret_cast<const char *>(rep.layout.data()), (std::streamsize)(sizeof(ck_iso3_t) * rep.layout.size()));
        o.write(reinterpret_cast<const char *>(rep.sightings.data()), (std::streamsize)(sizeof(int32_t) * rep.sightings.size()));
        o.write(reinterpret_cast<const char *>(rep.tag_rms.data()), (std::streamsize)(sizeof(double) * rep.tag_rms.size()));
        for (const auto &P : rep.poses) o.write(reinterpret_cast<const char *>(P.data()), sizeof(double) * 12);
        std::printf("%s %d iterations, status %d\n", got ? "OK" : "NONE", rep.result.iters, rep.result.status);
        fc.clear();
        return fc.steps() == 0 ? 0 : 1;
    } catch (const chalkydri::Panic &e) {
        std::fprintf(stderr, "panic: %s\n", e.what());
        return 3;
    }
}
