// rig_refine_demo — the C++ host layer of the rig pose refinement (include/chalkydri.hpp: RigSolver::refine), driven from
// tests/test_cpp_rig_refine.py.
//   rig_refine_demo host  IN OUT   solve_robust, then refine (six unknowns, heading prior 0.01 rad, the robust solve's masks) on the host, the
//                                  refined records to OUT
//   rig_refine_demo batch IN OUT   the same on a handle of its own
//   rig_refine_demo host_no_heading IN OUT   on the host without the prior and without the masks, RigSolver::refine given no headings at all
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
        if (at + sizeof v > buf.size()) throw Panic("rig_refine_demo: input too short");
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
    if (argc != 4) { std::fprintf(stderr, "usage: rig_refine_demo host|batch IN OUT\n"); return 2; }
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
        if (mode != "host" && mode != "batch" && mode != "host_no_heading") throw Panic("rig_refine_demo: unknown mode " + mode);
        const bool host = mode != "batch";
        RigSolver solver = host ? RigSolver() : RigSolver(std::make_shared<Handle>(64, 64, 1, std::vector<std::string>{"tag36h11"}, 3, 1, 0));
        const std::vector<ck_rig_robust_result_t> fused = solver.solve_robust(steps, gyro, RigSolver::robust_defaults(), host);
        std::vector<ck_rig_result_t> start;
        std::vector<uint64_t> rejected;
        for (const auto &f : fused) {
            start.push_back(f.fused);
            rejected.insert(rejected.end(), f.rejected, f.rejected + CK_RIG_MAX_CAMS);
        }
        ck_rig_refine_params_t prm = RigSolver::refine_defaults();
        prm.mode = CK_RIG_REFINE_FREE; prm.gyro_sigma_rad = 0.01; prm.max_iters = 30;
        if (mode == "host_no_heading") prm.gyro_sigma_rad = 0.0;
        const std::vector<ck_rig_refined_t> res = mode == "host_no_heading" ? solver.refine(steps, std::vector<double>(), start, prm, true)
                                                                            : solver.refine(steps, gyro, start, prm, host, &rejected);
        std::ofstream out(argv[3], std::ios::binary);
        out.write(reinterpret_cast<const char *>(res.data()), (std::streamsize)(res.size() * sizeof(ck_rig_refined_t)));
        int posed = 0;
        for (const auto &r : res) posed += r.status <= CK_RIG_REFINE_MAXITERS;
        std::printf("OK %d of %d\n", posed, n);
        return 0;
    } catch (const Panic &p) {
        std::fprintf(stderr, "panic: %s\n", p.what());
        return 3;
    }
}
