// rig_robust_host_check — the host twin of the robust rig solve (ck_rig_host.c: ck_rig_solve_robust_host) as a stand-alone program
// under AddressSanitizer + UBSan, driven from tests/test_cpp_rig_robust.py: the program is linked with the one C file, not with the
// library, and exits non-zero on the first finding of either sanitizer.
//   rig_robust_host_check IN OUT
// IN is rig_demo's: int32 n, int32 n_cams, then per step and camera int32 n_tags, robot_to_cam [7], n_tags tags [7], 4 * n_tags
// bearings [3]; then n gyro headings.  OUT: the n records.  Every step is solved three times: in the batch, alone (its arrays
// allocated to the byte, so that a read past a step's own tags or bearings is a finding), and alone with min_inlier_tags above what
// it has.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "chalkydri_hip.h"

struct Reader {
    std::vector<char> buf;
    size_t at = 0;
    bool ok = true;
    template <typename T>
    T get() {
        T v{};
        if (at + sizeof v > buf.size()) { ok = false; return v; }
        std::memcpy(&v, buf.data() + at, sizeof v);
        at += sizeof v;
        return v;
    }
    ck_iso3_t iso() {
        ck_iso3_t r;
        for (double &v : r.t) v = get<double>();
        for (double &v : r.q) v = get<double>();
        return r;
    }
};

int main(int argc, char **argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: rig_robust_host_check IN OUT\n"); return 2; }
    std::ifstream in(argv[1], std::ios::binary);
    Reader rd{std::vector<char>(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>())};
    const int n = rd.get<int32_t>(), n_cams = rd.get<int32_t>();
    if (!rd.ok || n < 1 || n_cams < 1 || n_cams > CK_RIG_MAX_CAMS) { std::fprintf(stderr, "bad input\n"); return 2; }
    std::vector<ck_sqpnp_problem_t> probs((size_t)n_cams * n);
    std::vector<ck_iso3_t> tags;
    std::vector<double> b;
    for (int s = 0; s < n; s++)
        for (int c = 0; c < n_cams; c++) {
            ck_sqpnp_problem_t &p = probs[(size_t)c * n + s];
            p = ck_sqpnp_problem_t{};
            p.n_tags = rd.get<int32_t>(); p.n_bearings = 4 * p.n_tags;
            p.tag_offset = (int32_t)tags.size(); p.bearing_offset = (int32_t)(b.size() / 3);
            p.robot_to_cam = rd.iso();
            for (int t = 0; t < p.n_tags; t++) tags.push_back(rd.iso());
            for (int k = 0; k < 12 * p.n_tags; k++) b.push_back(rd.get<double>());
        }
    std::vector<double> gyro(n);
    for (double &g : gyro) g = rd.get<double>();
    if (!rd.ok) { std::fprintf(stderr, "input too short\n"); return 2; }
    ck_rig_robust_params_t prm;
    ck_rig_robust_params_default(&prm);
    std::vector<ck_rig_robust_result_t> out(n);
    int rc = ck_rig_solve_robust_host(&prm, n_cams, probs.data(), n, tags.data(), (int32_t)tags.size(), b.data(), (int32_t)(b.size() / 3),
                                      gyro.data(), out.data());
    if (rc != CK_OK) { std::fprintf(stderr, "batch: rc %d\n", rc); return 1; }
    int rejected = 0;
    for (int s = 0; s < n; s++) {
        std::vector<ck_sqpnp_problem_t> one(n_cams);
        std::vector<ck_iso3_t> t1;
        std::vector<double> b1;
        for (int c = 0; c < n_cams; c++) {
            const ck_sqpnp_problem_t &p = probs[(size_t)c * n + s];
            one[c] = p;
            one[c].tag_offset = (int32_t)t1.size(); one[c].bearing_offset = (int32_t)(b1.size() / 3);
            t1.insert(t1.end(), tags.begin() + p.tag_offset, tags.begin() + p.tag_offset + p.n_tags);
            b1.insert(b1.end(), b.begin() + 3 * (size_t)p.bearing_offset, b.begin() + 3 * ((size_t)p.bearing_offset + p.n_bearings));
        }
        t1.shrink_to_fit(); b1.shrink_to_fit();
        ck_rig_robust_result_t r;
        rc = ck_rig_solve_robust_host(&prm, n_cams, one.data(), 1, t1.data(), (int32_t)t1.size(), b1.data(), (int32_t)(b1.size() / 3), &gyro[s], &r);
        if (rc != CK_OK || std::memcmp(&r, &out[s], sizeof r) != 0) { std::fprintf(stderr, "step %d alone: rc %d or other bytes\n", s, rc); return 1; }
        rejected += r.n_rejected;
        ck_rig_robust_params_t q = prm;
        q.min_inlier_tags = r.fused.n_tags + 1;
        rc = ck_rig_solve_robust_host(&q, n_cams, one.data(), 1, t1.data(), (int32_t)t1.size(), b1.data(), (int32_t)(b1.size() / 3), &gyro[s], &r);
        if (rc != CK_OK || (t1.size() && r.status != CK_RIG_ROBUST_NO_CONSENSUS) || r.fused.valid) {
            std::fprintf(stderr, "step %d: no NO_CONSENSUS\n", s);
            return 1;
        }
    }
    prm.mu_factor = 1.0;
    if (ck_rig_solve_robust_host(&prm, n_cams, probs.data(), n, tags.data(), (int32_t)tags.size(), b.data(), (int32_t)(b.size() / 3), gyro.data(),
                                 out.data()) != CK_EINVAL) { std::fprintf(stderr, "mu_factor 1 was taken\n"); return 1; }
    std::ofstream o(argv[2], std::ios::binary);
    o.write(reinterpret_cast<const char *>(out.data()), (std::streamsize)(out.size() * sizeof(ck_rig_robust_result_t)));
    std::printf("OK %d steps, %d rejected\n", n, rejected);
    return 0;
}
