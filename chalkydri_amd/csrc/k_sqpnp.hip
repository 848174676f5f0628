// k_sqpnp.hip — batched SQPnP robot-pose solve, OpenCV-5 unprojection and the AprilTags::process glue.
//
// Replaces chalkydri_sqpnp::SqPnP::solve_robot_pose (crates/chalkydri_sqpnp/src/lib.rs:297-377, with solve :248-295,
// build_linear_system :124-180, solve_rotation_candidates :396-428, optimization :463-480, nearest_so3 :42-59) and
// the per-frame glue of crates/apriltags/src/lib.rs:293-379.  All arithmetic is f64.
//
// Two waves per problem.  The work is ~0.3 MFLOP and latency-bound, so the mapping favours determinism over peak rate:
// every entry of Q_rr/Q_rt/Q_tt is accumulated by ONE lane over the points in index order (same sums as the scalar code,
// no atomics, no reduction tree); the 9x9 Jacobi eigen-decomposition runs its rotations with 9 lanes updating one
// row/column element each; the six SQP refinements run as six groups of 16 lanes, each lane holding one row of the 15x15
// KKT system in registers (LU with partial pivoting: pivot rows travel by shuffle, rows are never moved); the cheirality
// test of the winner selection is spread over a wave.  MFMA is deliberately not used: the only contraction,
// (9 x 3N)(3N x 9) with N <= 120, is 0.2 MFLOP — see DESIGN.md.
#include <math.h>
#include <string.h>

#include <vector>

#include "ck_internal.h"
#include "ck_mat3.h"
#include "ck_sqpnp_dev.h"

namespace {

struct SolveArgs {
    ck_sqpnp_params_t prm;
    const ck_sqpnp_problem_t *problems;
    const ck_iso3_t *tags;
    const double *bearings;
    ck_sqpnp_result_t *out;
    int n;
    int max_points; // capacity of the per-problem world-point scratch
    double *world;  // [n][max_points][3]
};

constexpr int SQ_NT = 128; // two waves: six candidate groups of 16 lanes in the refinement, 128-wide loops elsewhere
__global__ __launch_bounds__(SQ_NT) void k_sqpnp(SolveArgs a) {
    __shared__ double sQrr[81], sQrt[27], sQtt[9], sQttInv[9], sOmega[81], sA[81], sV[81], sW[9];
    __shared__ double sCandR[6][9], sCandE[6];
    __shared__ double sCentroid[3], sRot[2];
    __shared__ int sIdx[9];
    const int lane = threadIdx.x, pi = blockIdx.x;
    if (pi >= a.n) return;
    const ck_sqpnp_problem_t pr = a.problems[pi];
    ck_sqpnp_result_t *res = &a.out[pi];
    const int n_tags = pr.n_tags, n = 4 * pr.n_tags;
    if (lane == 0) { res->valid = 0; res->pad = 0; }
    if (n < 3 || n != pr.n_bearings || n > a.max_points) return; // lib.rs:255
    const ck_iso3_t *tags = a.tags + pr.tag_offset;
    const double *p2 = a.bearings + (size_t)3 * pr.bearing_offset;
    double *world = a.world + (size_t)pi * a.max_points * 3;
    for (int i = lane; i < n; i += SQ_NT) {
        int t = i >> 2, c = i & 3;
        double R[9];
        quat_to_mat(tags[t].q, R);
        ckp_tag_corner(R, tags[t].t, c, world + i * 3);
    }
    __syncthreads();
    if (lane < 3) { // centroid: index order, like the fold in lib.rs:259-260
        double s = 0;
        for (int i = 0; i < n; i++) s += world[i * 3 + lane];
        sCentroid[lane] = s / (double)n;
    }
    __syncthreads();
    // build_linear_system (lib.rs:124-180): entry e of [Q_rr(81) | Q_rt(27) | Q_tt(9)] belongs to one lane
    for (int e = lane; e < 117; e += SQ_NT) {
        double acc = 0;
        for (int k = 0; k < n; k++) {
            const double *v = p2 + 3 * k;
            double X[3] = {world[k * 3] - sCentroid[0], world[k * 3 + 1] - sCentroid[1], world[k * 3 + 2] - sCentroid[2]};
            double sq = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
            double inv = 1.0 / sq;
            if (e < 81) {
                int row = e / 9, col = e - row * 9;
                int ai = row / 3, i = row - ai * 3, bi = col / 3, j = col - bi * 3;
                double P = (i == j ? 1.0 : 0.0) - (v[i] * v[j]) * inv;
                acc += (P * X[ai]) * X[bi];
            } else if (e < 108) {
                int q = e - 81, row = q / 3, j = q - row * 3;
                int ai = row / 3, i = row - ai * 3;
                double P = (i == j ? 1.0 : 0.0) - (v[i] * v[j]) * inv;
                acc += P * X[ai];
            } else {
                int q = e - 108, i = q / 3, j = q - i * 3;
                acc += (i == j ? 1.0 : 0.0) - (v[i] * v[j]) * inv;
            }
        }
        if (e < 81) sQrr[e] = acc; else if (e < 108) sQrt[e - 81] = acc; else sQtt[e - 108] = acc;
    }
    __syncthreads();
    if (lane == 0) {
        double inv[9];
        if (!mat3_try_inverse(sQtt, inv)) for (int i = 0; i < 9; i++) inv[i] = 0.0; // unwrap_or_default (lib.rs:171)
        for (int i = 0; i < 9; i++) sQttInv[i] = inv[i];
    }
    __syncthreads();
    for (int e = lane; e < 81; e += SQ_NT) {
        int i = e / 9, j = e - i * 9;
        double t0 = sQrt[i * 3] * sQttInv[0] + sQrt[i * 3 + 1] * sQttInv[3] + sQrt[i * 3 + 2] * sQttInv[6];
        double t1 = sQrt[i * 3] * sQttInv[1] + sQrt[i * 3 + 1] * sQttInv[4] + sQrt[i * 3 + 2] * sQttInv[7];
        double t2 = sQrt[i * 3] * sQttInv[2] + sQrt[i * 3 + 1] * sQttInv[5] + sQrt[i * 3 + 2] * sQttInv[8];
        double om = sQrr[e] - (t0 * sQrt[j * 3] + t1 * sQrt[j * 3 + 1] + t2 * sQrt[j * 3 + 2]);
        sOmega[e] = om; sA[e] = om; sV[e] = (i == j) ? 1.0 : 0.0;
    }
    __syncthreads();
    jacobi9_wave(sA, sV, lane); // symmetric eigen-decomposition of Omega (ck_sqpnp_dev.h)
    __syncthreads();
    if (lane == 0) {
        for (int i = 0; i < 9; i++) { sW[i] = sA[i * 9 + i]; sIdx[i] = i; }
        for (int i = 1; i < 9; i++) { // stable ascending order of eigenvalues (lib.rs:400-401)
            int v = sIdx[i], j = i - 1;
            while (j >= 0 && sW[sIdx[j]] > sW[v]) { sIdx[j + 1] = sIdx[j]; j--; }
            sIdx[j + 1] = v;
        }
        sRot[0] = cos(pr.gyro); sRot[1] = sin(pr.gyro);
    }
    __syncthreads();
    double Rrc[9];
    quat_to_mat(pr.robot_to_cam.q, Rrc);
    const double fwd[3] = {Rrc[0], Rrc[3], Rrc[6]}; // column 0 (lib.rs:313-318)
    {   // solve_rotation_candidates (lib.rs:403-425): group g of 16 lanes = candidate 2*t + sign index
        const int g = lane >> 4, gl = lane & 15;
        if (g < 6) {
            int t = g >> 1;
            double sign = (g & 1) ? 1.0 : -1.0, guess[9], r[9];
            for (int k = 0; k < 9; k++) guess[k] = sV[k * 9 + sIdx[t]] * sign;
            nearest_so3(guess, r);
            double energy = optimization16<false>(a.prm.max_iter, a.prm.tol_sq, r, sOmega, nullptr, gl);
            double fx = r[0] * fwd[0] + r[1] * fwd[1] + r[2] * fwd[2];
            double fy = r[3] * fwd[0] + r[4] * fwd[1] + r[5] * fwd[2];
            double dot = fx * sRot[0] + fy * sRot[1];
            double ae = 1.0 - dot;
            if (ae < 0.0) ae = 0.0;
            energy += pr.sign_change_error * ae;
            if (gl == 0) {
                for (int k = 0; k < 9; k++) sCandR[g][k] = r[k];
                sCandE[g] = energy;
            }
        }
    }
    __syncthreads();
    if (lane >= 64) return; // the first wave picks the winner: every lane replays the (cheap) selection, the cheirality test
                            // over the points is spread over the lanes
    int order[6] = {0, 1, 2, 3, 4, 5};
    for (int i = 1; i < 6; i++) { // stable sort by penalised energy (lib.rs:427)
        int v = order[i], j = i - 1;
        while (j >= 0 && sCandE[order[j]] > sCandE[v]) { order[j + 1] = order[j]; j--; }
        order[j + 1] = v;
    }
    bool found = false;
    double best_score = DBL_MAX, bestR[9], bestT[3], best_energy = 0;
    for (int oi = 0; oi < 6; oi++) {
        const double *r = sCandR[order[oi]];
        double Rm[9];
        for (int c = 0; c < 3; c++)
            for (int rr = 0; rr < 3; rr++) Rm[rr * 3 + c] = r[c * 3 + rr];
        double qtr[3], tl[3], Rc[3], t[3];
        for (int j = 0; j < 3; j++) {
            double s = 0;
            for (int i = 0; i < 9; i++) s += sQrt[i * 3 + j] * r[i];
            qtr[j] = s;
        }
        mat3_vec(sQttInv, qtr, tl);
        mat3_vec(Rm, sCentroid, Rc);
        for (int k = 0; k < 3; k++) t[k] = -tl[k] - Rc[k];
        bool behind = false;
        for (int i = lane; i < n; i += 64) {
            double pc[3];
            mat3_vec(Rm, world + 3 * i, pc);
            if (!(pc[2] + t[2] > 0.0)) behind = true;
        }
        if (__ballot(behind)) continue; // uniform: all points must be in front (lib.rs:276-283)
        if (sCandE[order[oi]] < best_score) {
            best_score = sCandE[order[oi]];
            double e = 0;
            for (int i = 0; i < 9; i++) {
                double s = 0;
                for (int j = 0; j < 9; j++) s += sOmega[i * 9 + j] * r[j];
                e += r[i] * s;
            }
            best_energy = e;
            polar_rotation(Rm, bestR); // Rot3::from_matrix (lib.rs:289)
            for (int k = 0; k < 3; k++) bestT[k] = t[k];
            found = true;
        }
    }
    if (!found || lane != 0) return;
    double distance = sqrt(bestT[0] * bestT[0] + bestT[1] * bestT[1] + bestT[2] * bestT[2]);
    ckp_std_devs(best_energy, n_tags, distance, res->std_devs);
    // world_to_cam^-1 * robot_to_cam, then the yaw pivot about the tag centroid (lib.rs:328-376)
    double Rt[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) Rt[i * 3 + j] = bestR[j * 3 + i];
    double d[3] = {pr.robot_to_cam.t[0] - bestT[0], pr.robot_to_cam.t[1] - bestT[1], pr.robot_to_cam.t[2] - bestT[2]};
    double robot_pos[3], robot_rot[9];
    mat3_vec(Rt, d, robot_pos);
    mat3_mul(Rt, Rrc, robot_rot);
    double tc[3] = {0, 0, 0};
    for (int t = 0; t < n_tags; t++)
        for (int k = 0; k < 3; k++) tc[k] += tags[t].t[k];
    for (int k = 0; k < 3; k++) tc[k] /= (double)n_tags;
    double yaw;
    ckp_yaw_pivot(robot_rot, robot_pos, tc, pr.gyro, res->rot, res->pos, &yaw);
    res->yaw = yaw;
    res->energy = best_energy;
    res->valid = 1;
}

__global__ void k_unproject(ck_opencv5_t cam, const double *px, int n, double *bearings, uint8_t *ok) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double b[3];
    bool good = unproject_one(cam, px[2 * i], px[2 * i + 1], b);
    bearings[3 * i] = b[0]; bearings[3 * i + 1] = b[1]; bearings[3 * i + 2] = b[2];
    ok[i] = good ? 1 : 0;
}
// ... of any camera model (ck_camera_unproject): the bytes of ck_camera_unproject_host
__global__ void k_camera_unproject(ck_camera_t cam, const double *px, int n, double *bearings, uint8_t *ok) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double b[3];
    bool good = camera_unproject_one(cam, px[2 * i], px[2 * i + 1], b);
    bearings[3 * i] = b[0]; bearings[3 * i + 1] = b[1]; bearings[3 * i + 2] = b[2];
    ok[i] = good ? 1 : 0;
}

// AprilTags::process glue, one thread per frame: known-tag filter + unprojection -> one SQPnP problem per frame
struct GlueArgs {
    ck_stage_ws ws;
    ck_camera_t cam; // the params' OpenCVModel5 or the handle's camera (ck_kernel_camera)
    ck_iso3_t robot_to_cam;
    const ck_field_tag_t *field; int n_field;
    const double *gyro; const uint8_t *has_gyro;
    double sign_change_error;
    const ck_dev_family *fams; int allow_unverified; // ids past a family's verified prefix are not upstream ids (ck_family_t.n_upstream)
    ck_sqpnp_problem_t *problems; ck_iso3_t *tags; double *bearings; // per frame: det_cap tags, 4*det_cap bearings
    int n;
};
__global__ void k_glue(GlueArgs a) {
    int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= a.n) return;
    const ck_stage_ws &ws = a.ws;
    uint32_t nd = ws.d_counters[(size_t)f * CK_CNT_STRIDE + CK_CNT_DETS];
    const ck_detection_t *dets = ws.d_dets + (size_t)f * ws.det_cap;
    ck_iso3_t *tags = a.tags + (size_t)f * ws.det_cap;
    double *bear = a.bearings + (size_t)f * ws.det_cap * 12;
    int nt = 0;
    if (nd > 0 && a.has_gyro[f]) {
        for (uint32_t i = 0; i < nd; i++) {
            int k = -1;
            for (int j = 0; j < a.n_field; j++)
                if (a.field[j].id == dets[i].id) { k = j; break; }
            if (k < 0) continue; // unknown tag (apriltags/src/lib.rs:306-308)
            if (!a.allow_unverified && (uint32_t)dets[i].id >= a.fams[dets[i].family].n_upstream) continue; // not an upstream id
            double b[12];
            bool ok = true;
            for (int c = 0; c < 4; c++) ok = camera_unproject_one(a.cam, dets[i].p[c][0], dets[i].p[c][1], b + 3 * c) && ok;
            if (!ok) continue; // lib.rs:324
            tags[nt] = a.field[k].pose;
            for (int q = 0; q < 12; q++) bear[nt * 12 + q] = b[q];
            nt++;
        }
    }
    ck_sqpnp_problem_t pr;
    pr.n_tags = nt; pr.n_bearings = 4 * nt;
    pr.tag_offset = f * ws.det_cap; pr.bearing_offset = f * ws.det_cap * 4;
    pr.robot_to_cam = a.robot_to_cam; pr.gyro = a.gyro[f]; pr.sign_change_error = a.sign_change_error;
    a.problems[f] = pr;
}
__global__ void k_measure(ck_stage_ws ws, const ck_sqpnp_result_t *res, uint8_t camera_id, ck_vision_measurement_t *out, int32_t *valid, int n) {
    int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    ck_vision_measurement_t m;
    memset(&m, 0, sizeof m);
    m.camera_id = camera_id;
    int ok = res[f].valid;
    if (ok) {
        uint32_t nd = ws.d_counters[(size_t)f * CK_CNT_STRIDE + CK_CNT_DETS];
        m.pose_x = res[f].pos[0]; m.pose_y = res[f].pos[1]; m.pose_rot = res[f].yaw;
        m.std_x = res[f].std_devs[0]; m.std_y = res[f].std_devs[1]; m.std_rot = res[f].std_devs[2];
        m.tag_count = (uint8_t)(nd > 255 ? 255 : nd); // ALL detections (lib.rs:354)
    }
    out[f] = m;
    valid[f] = ok;
}

} // namespace

extern "C" int ck_sqpnp_solve_batch(ck_handle_t *h, const ck_sqpnp_params_t *params, const ck_sqpnp_problem_t *problems, int32_t n,
                                    const ck_iso3_t *tags, int32_t n_tags_total, const double *bearings, int32_t n_bearings_total,
                                    ck_sqpnp_result_t *out) {
    if (!h || !params || !problems || !out || n < 0 || n_tags_total < 0 || n_bearings_total < 0 || (n_tags_total > 0 && !tags) ||
        (n_bearings_total > 0 && !bearings)) return CK_EINVAL;
    if (n == 0) return CK_OK;
    int max_pts = 4;
    for (int i = 0; i < n; i++) {
        const ck_sqpnp_problem_t &p = problems[i];
        if (p.n_tags < 0 || p.n_bearings < 0 || p.tag_offset < 0 || p.bearing_offset < 0 || (int64_t)p.tag_offset + p.n_tags > n_tags_total ||
            (int64_t)p.bearing_offset + p.n_bearings > n_bearings_total) return CK_EINVAL;
        if (4 * p.n_tags > max_pts) max_pts = 4 * p.n_tags;
    }
    CK_HIP(hipSetDevice(h->device));
    DevBuf<ck_sqpnp_problem_t> dp; DevBuf<ck_iso3_t> dt; DevBuf<double> db, dw; DevBuf<ck_sqpnp_result_t> dr;
    if (dp.alloc((size_t)n) || dt.alloc((size_t)n_tags_total) || db.alloc((size_t)3 * n_bearings_total) || dw.alloc((size_t)n * max_pts * 3) || dr.alloc((size_t)n)) return CK_ENOMEM;
    CK_HIP(hipMemcpyAsync(dp.p, problems, sizeof(ck_sqpnp_problem_t) * (size_t)n, hipMemcpyHostToDevice, h->stream));
    if (n_tags_total) CK_HIP(hipMemcpyAsync(dt.p, tags, sizeof(ck_iso3_t) * (size_t)n_tags_total, hipMemcpyHostToDevice, h->stream));
    if (n_bearings_total) CK_HIP(hipMemcpyAsync(db.p, bearings, sizeof(double) * 3 * (size_t)n_bearings_total, hipMemcpyHostToDevice, h->stream));
    SolveArgs a;
    a.prm = *params; a.problems = dp.p; a.tags = dt.p; a.bearings = db.p; a.out = dr.p; a.n = n; a.max_points = max_pts; a.world = dw.p;
    hipLaunchKernelGGL(k_sqpnp, dim3((unsigned)n), dim3(SQ_NT), 0, h->stream, a);
    CK_HIP(hipGetLastError());
    CK_HIP(hipMemcpyAsync(out, dr.p, sizeof(ck_sqpnp_result_t) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    CK_HIP(hipStreamSynchronize(h->stream));
    return CK_OK;
}

extern "C" void ck_sqpnp_create_solver_camera_transform(double fwd_m, double left_m, double up_m, double roll_deg, double pitch_deg,
                                                        double yaw_deg, ck_iso3_t *out) {
    // lib.rs:430-461 — construction-time host arithmetic (the reference calls it once in AprilTags::new)
    const double D2R = PI_D / 180.0;
    double r = roll_deg * D2R, p = pitch_deg * D2R, y = yaw_deg * D2R;
    double cr = cos(r * 0.5), sr = sin(r * 0.5), cp = cos(p * 0.5), sp = sin(p * 0.5), cy = cos(y * 0.5), sy = sin(y * 0.5);
    double qw = cr * cp * cy + sr * sp * sy, qx = sr * cp * cy - cr * sp * sy, qy = cr * sp * cy + sr * cp * sy, qz = cr * cp * sy - sr * sp * cy;
    double Rn[9] = {1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw),
                    2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw),
                    2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)};
    const double C[9] = {0, 0, 1, -1, 0, 0, 0, -1, 0}; // nwu -> cv
    double Rc[9], Ri[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) Rc[i * 3 + j] = Rn[i * 3] * C[j] + Rn[i * 3 + 1] * C[3 + j] + Rn[i * 3 + 2] * C[6 + j];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) Ri[i * 3 + j] = Rc[j * 3 + i];
    double T[3] = {fwd_m, left_m, up_m};
    for (int i = 0; i < 3; i++) out->t[i] = -(Ri[i * 3] * T[0] + Ri[i * 3 + 1] * T[1] + Ri[i * 3 + 2] * T[2]);
    double tr = Ri[0] + Ri[4] + Ri[8], q[4];
    if (tr > 0) { double s = sqrt(tr + 1.0) * 2; q[0] = 0.25 * s; q[1] = (Ri[7] - Ri[5]) / s; q[2] = (Ri[2] - Ri[6]) / s; q[3] = (Ri[3] - Ri[1]) / s; }
    else if (Ri[0] > Ri[4] && Ri[0] > Ri[8]) { double s = sqrt(1.0 + Ri[0] - Ri[4] - Ri[8]) * 2; q[0] = (Ri[7] - Ri[5]) / s; q[1] = 0.25 * s; q[2] = (Ri[1] + Ri[3]) / s; q[3] = (Ri[2] + Ri[6]) / s; }
    else if (Ri[4] > Ri[8]) { double s = sqrt(1.0 + Ri[4] - Ri[0] - Ri[8]) * 2; q[0] = (Ri[2] - Ri[6]) / s; q[1] = (Ri[1] + Ri[3]) / s; q[2] = 0.25 * s; q[3] = (Ri[5] + Ri[7]) / s; }
    else { double s = sqrt(1.0 + Ri[8] - Ri[0] - Ri[4]) * 2; q[0] = (Ri[3] - Ri[1]) / s; q[1] = (Ri[2] + Ri[6]) / s; q[2] = (Ri[5] + Ri[7]) / s; q[3] = 0.25 * s; }
    for (int i = 0; i < 4; i++) out->q[i] = q[i];
}

extern "C" int ck_unproject_opencv5(const ck_opencv5_t *cam, const double *px, int32_t n, double *bearings, uint8_t *ok) {
    if (!cam || !px || !bearings || !ok || n < 0) return CK_EINVAL;
    if (n == 0) return CK_OK;
    if (ck_device_count() <= 0) return CK_ENODEVICE;
    DevBuf<double> dpx, db; DevBuf<uint8_t> dok;
    if (dpx.alloc((size_t)2 * n) || db.alloc((size_t)3 * n) || dok.alloc((size_t)n)) return CK_ENOMEM;
    CK_HIP(hipMemcpy(dpx.p, px, sizeof(double) * 2 * (size_t)n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_unproject, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, 0, *cam, dpx.p, n, db.p, dok.p);
    CK_HIP(hipGetLastError());
    CK_HIP(hipMemcpy(bearings, db.p, sizeof(double) * 3 * (size_t)n, hipMemcpyDeviceToHost));
    CK_HIP(hipMemcpy(ok, dok.p, (size_t)n, hipMemcpyDeviceToHost));
    return CK_OK;
}

extern "C" int ck_camera_unproject(const ck_camera_t *cam, const double *px, int32_t n, double *bearings, uint8_t *ok) {
    const int rc = ck_camera_check(cam);
    if (rc != CK_OK) return rc;
    if (!px || !bearings || !ok || n < 0) return CK_EINVAL;
    if (n == 0) return CK_OK;
    if (ck_device_count() <= 0) return CK_ENODEVICE;
    ck_camera_t c = *cam;
    ckm_effective(cam->model, cam->k, c.k);
    DevBuf<double> dpx, db; DevBuf<uint8_t> dok;
    if (dpx.alloc((size_t)2 * n) || db.alloc((size_t)3 * n) || dok.alloc((size_t)n)) return CK_ENOMEM;
    CK_HIP(hipMemcpy(dpx.p, px, sizeof(double) * 2 * (size_t)n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_camera_unproject, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, 0, c, dpx.p, n, db.p, dok.p);
    CK_HIP(hipGetLastError());
    CK_HIP(hipMemcpy(bearings, db.p, sizeof(double) * 3 * (size_t)n, hipMemcpyDeviceToHost));
    CK_HIP(hipMemcpy(ok, dok.p, (size_t)n, hipMemcpyDeviceToHost));
    return CK_OK;
}

extern "C" int ck_set_camera(ck_handle_t *h, const ck_camera_t *cam) {
    if (!h) return CK_EINVAL;
    if (!cam) { h->has_camera = 0; return CK_OK; }
    const int rc = ck_camera_check(cam);
    if (rc != CK_OK) return rc; // (the previous setting stays)
    h->camera = *cam;
    ckm_effective(cam->model, cam->k, h->camera.k);
    h->has_camera = 1;
    return CK_OK;
}

// k_sqpnp once more on the problems the handle's last ck_process_* call left in its workspace, on `stream` (ck_rig_time_last: what the
// per-camera path pays for the solve).  It rewrites ws.d_results with the same values.
int ck_launch_sqpnp_last(ck_handle *h, int n, const ck_sqpnp_params_t *prm, hipStream_t stream) {
    if (n < 1 || n > h->cfg.max_batch) return CK_EINVAL;
    const ck_stage_ws &ws = h->ws;
    SolveArgs a;
    a.prm = *prm; a.problems = ws.d_problems; a.tags = ws.d_pose_tags; a.bearings = ws.d_bearings; a.out = ws.d_results; a.n = n;
    a.max_points = ws.det_cap * 4; a.world = ws.d_world;
    hipLaunchKernelGGL(k_sqpnp, dim3((unsigned)n), dim3(SQ_NT), 0, stream, a);
    CK_HIP(hipGetLastError());
    return CK_OK;
}

// detect (already run) -> glue -> solve -> measurement, all on the device; only 64-byte records come back
int ck_run_pose(ck_handle *h, int n, const ck_process_params_t *pp, const double *gyro, const uint8_t *has_gyro,
                ck_vision_measurement_t *out, int32_t *valid, bool upload_field, bool sync) {
    ck_stage_ws &ws = h->ws;
    if (pp->n_field > ws.field_cap) return CK_ECAPACITY;
    // gyro / has_gyro / out / valid may be host or device pointers (hipMemcpyDefault resolves them)
    if (pp->n_field && upload_field) CK_HIP(hipMemcpyAsync(ws.d_field, pp->field, sizeof(ck_field_tag_t) * (size_t)pp->n_field, hipMemcpyDefault, h->stream));
    CK_HIP(hipMemcpyAsync(ws.d_gyro, gyro, sizeof(double) * (size_t)n, hipMemcpyDefault, h->stream));
    CK_HIP(hipMemcpyAsync(ws.d_has_gyro, has_gyro, (size_t)n, hipMemcpyDefault, h->stream));
    GlueArgs g;
    g.ws = ws; g.cam = ck_kernel_camera(h, pp->cam); g.robot_to_cam = pp->robot_to_cam; g.field = ws.d_field; g.n_field = pp->n_field; g.gyro = ws.d_gyro;
    g.fams = h->d_fams; g.allow_unverified = pp->allow_unverified_ids;
    g.has_gyro = ws.d_has_gyro; g.sign_change_error = pp->sign_change_error; g.problems = ws.d_problems; g.tags = ws.d_pose_tags;
    g.bearings = ws.d_bearings; g.n = n;
    hipLaunchKernelGGL(k_glue, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, h->stream, g);
    SolveArgs a;
    a.prm = pp->sqpnp; a.problems = ws.d_problems; a.tags = ws.d_pose_tags; a.bearings = ws.d_bearings; a.out = ws.d_results; a.n = n;
    a.max_points = ws.det_cap * 4; a.world = ws.d_world;
    hipLaunchKernelGGL(k_sqpnp, dim3((unsigned)n), dim3(SQ_NT), 0, h->stream, a);
    hipLaunchKernelGGL(k_measure, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, h->stream, ws, ws.d_results, pp->camera_id, ws.d_meas, ws.d_valid, n);
    CK_HIP(hipGetLastError());
    CK_HIP(hipMemcpyAsync(out, ws.d_meas, sizeof(ck_vision_measurement_t) * (size_t)n, hipMemcpyDefault, h->stream));
    CK_HIP(hipMemcpyAsync(valid, ws.d_valid, sizeof(int32_t) * (size_t)n, hipMemcpyDefault, h->stream));
    if (sync) CK_HIP(hipStreamSynchronize(h->stream));
    return CK_OK;
}
