// rig_robust_demo — the C++ host layer of the robust camera rig (include/chalkydri.hpp: RigSolver::solve_robust), driven from
// tests/test_cpp_rig_robust.py.
//   rig_robust_demo host  IN OUT   solve_robust on the host (no device) on the steps of IN, the result records to OUT
//   rig_robust_demo batch IN OUT   solve_robust on a handle of its own
// IN is rig_demo's: int32 n, int32 n_cams, then per step and camera int32 n_tags, robot_to_cam [7], n_tags tags [7], 4 * n_tags
// bearings [3]; then n gyro headings.  Isometries are t[3], q[4] (w, x, y, z).
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
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
        if (at + sizeof v > buf.size()) throw Panic("rig_robust_demo: input too short");
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

int main(int argc, char **argv) {
    if (argc != 4) { std::fprintf(stderr, "usage: rig_robust_demo host|batch IN OUT\n"); return 2; }
    try {
        const std::string mode = argv[1];
        std::ifstream in(argv[2], std::ios::binary);
        Reader rd{std::vector<char>(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>())};
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
        std::vector<ck_rig_robust_result_t> res;
        if (mode == "host") res = RigSolver().solve_robust(steps, gyro, RigSolver::robust_defaults(), true);
        else if (mode == "batch") res = RigSolver(std::make_shared<Handle>(64, 64, 1, std::vector<std::string>{"tag36h11"}, 3, 1, 0)).solve_robust(steps, gyro);
        else throw Panic("rig_robust_demo: unknown mode " + mode);
        std::ofstream out(argv[3], std::ios::binary);
        out.write(reinterpret_cast<const char *>(res.data()), (std::streamsize)(res.size() * sizeof(ck_rig_robust_result_t)));
        int valid = 0, rejected = 0;
        for (const auto &r : res) { valid += r.fused.valid; rejected += r.n_rejected; }
        std::printf("OK %d of %d, %d rejected\n", valid, n, rejected);
        return 0;
    } catch (const Panic &p) {
        std::fprintf(stderr, "panic: %s\n", p.what());
        return 3;
    }
}
