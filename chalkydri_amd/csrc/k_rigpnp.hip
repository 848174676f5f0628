// k_rigpnp.hip — one robot pose from all the cameras of a robot: batched SQPnP over rays with different origins.
//
// The unknown is world -> robot (R, t).  A bearing v of camera c (mounted by robot_to_cam = (A_c, b_c)) is the ray u = A_c^T v through
// o_c = -A_c^T b_c in the robot frame, and the cost sum_i (R X_i + t - o_i)^T M_i (R X_i + t - o_i), M_i = I - u_i u_i^T / u_i^T u_i,
// stays a quadratic in r = vec(R) once t is eliminated: E(r) = r^T Omega r - 2 g^T r + c.  So the kernel is k_sqpnp's with 13 more
// accumulated entries (q_r, q_t, q_0) and a linear term in the SQP step: one workgroup of two waves per time step, one lane per
// accumulated entry summing over cameras and points in index order, the wave-local Jacobi, six groups of 16 lanes for the
// refinements, the first wave for the winner with the cheirality test (each point in front of its OWN camera) spread over its lanes.
// ck_rig_host.c is the same arithmetic on the host.  All f64; no MFMA (the contraction is k_sqpnp's 0.2 MFLOP).
#include <math.h>
#include <string.h>

#include <vector>

#include "ck_internal.h"
#include "ck_mat3.h"
#include "ck_rig.h"
#include "ck_sqpnp_dev.h"

namespace {

struct RigCam {
    const ck_sqpnp_problem_t *problems; // [n] this camera's record of every step
    const ck_iso3_t *tags;
    const double *bearings;
    const uint32_t *counters;           // the handle's per-frame counters (detections for tag_count), or null
    int det_cap;                        // > 0: a handle's workspace, step s owns tags[s * det_cap ..] and bearings[s * det_cap * 4 ..] (the
                                        // records' offsets are relative to the piece of a split batch that wrote them); 0: the records' offsets
    int pad;
};
struct RigArgs {
    ck_rig_params_t prm;
    RigCam cam[CK_RIG_MAX_CAMS];
    int n_cams, n;
    int max_points;                     // capacity of a step in `points`
    int pad;
    const double *gyro;                 // [n]
    const uint8_t *has_gyro;            // [n], or null: every step has one
    double *points;                     // [n][max_points][CK_RIG_POINT_DOUBLES]
    ck_rig_result_t *out;               // [n]
    ck_vision_measurement_t *meas;      // [n] or null
    int32_t *valid;                     // [n] or null
};

constexpr int RIG_NT = 128;
constexpr int RIG_ENTRIES = 117 + 13 + 6; // Q_rr(81) | Q_rt(27) | Q_tt(9) | q_r(9) | q_t(3) | q_0 | scatter of the centred points (6)
__global__ __launch_bounds__(RIG_NT) void k_rig(RigArgs a) {
    __shared__ double sQrr[81], sQrt[27], sQtt[9], sQttInv[9], sOmega[81], sA[81], sV[81], sW[9];
    __shared__ double sQr[9], sQt[3], sQ0, sG[9], sC, sS[6], sNrm[3], sMu;
    __shared__ double sCandR[6][9], sCandE[6];
    __shared__ double sCentroid[3], sRot[2];
    __shared__ double sCamA[CK_RIG_MAX_CAMS][9], sCamB[CK_RIG_MAX_CAMS][3], sCamO[CK_RIG_MAX_CAMS][3];
    __shared__ long long sTagAt[CK_RIG_MAX_CAMS], sBearAt[CK_RIG_MAX_CAMS];
    __shared__ int sCnt[CK_RIG_MAX_CAMS], sBase[CK_RIG_MAX_CAMS + 1], sIdx[9], sOrder[6];
    const int lane = threadIdx.x, step = blockIdx.x;
    if (step >= a.n) return;
    ck_rig_result_t *res = &a.out[step];
    // the record of a step without a pose: all zero (and the heartbeat measurement).  The first wave writes it and lane 0 of the same
    // wave the pose at the end, so the stores to one address stay in order
    if (lane < (int)(sizeof(ck_rig_result_t) / 4)) reinterpret_cast<uint32_t *>(res)[lane] = 0u;
    if (lane == 0 && a.meas) {
        ck_vision_measurement_t m;
        memset(&m, 0, sizeof m);
        m.camera_id = a.prm.rig_id;
        a.meas[step] = m;
        a.valid[step] = 0;
    }
    if (lane < CK_RIG_MAX_CAMS) { // one lane per camera: its mount, its ray origin, its points of this step
        const int c = lane;
        int cnt = 0;
        if (c < a.n_cams) {
            const ck_sqpnp_problem_t *p = &a.cam[c].problems[step];
            const int nt = p->n_tags, cap = a.cam[c].det_cap;
            if (nt > 0 && (cap == 0 || nt <= cap)) cnt = 4 * nt;
            sTagAt[c] = cap > 0 ? (long long)step * cap : (long long)p->tag_offset;
            sBearAt[c] = cap > 0 ? (long long)step * cap * 4 : (long long)p->bearing_offset;
            double A[9];
            quat_to_mat(p->robot_to_cam.q, A);
            const double b[3] = {p->robot_to_cam.t[0], p->robot_to_cam.t[1], p->robot_to_cam.t[2]};
            for (int k = 0; k < 9; k++) sCamA[c][k] = A[k];
            for (int k = 0; k < 3; k++) {
                sCamB[c][k] = b[k];
                sCamO[c][k] = -(A[k] * b[0] + A[3 + k] * b[1] + A[6 + k] * b[2]);
            }
        }
        sCnt[c] = cnt;
    }
    __syncthreads();
    if (lane == 0) {
        int s = 0;
        for (int c = 0; c < CK_RIG_MAX_CAMS; c++) { sBase[c] = s; s += sCnt[c]; }
        sBase[CK_RIG_MAX_CAMS] = s;
    }
    __syncthreads();
    const int n = sBase[CK_RIG_MAX_CAMS], n_tags = n >> 2;
    const bool has_gyro = a.has_gyro ? a.has_gyro[step] != 0 : true;
    if (n < 3 || n > a.max_points || !has_gyro) return; // uniform: no tag in any camera, or "no gyro, no solve"
    const double gyro = a.gyro[step];
    double *pts = a.points + (size_t)step * a.max_points * CK_RIG_POINT_DOUBLES;
    const double cp[4][3] = {{0, -CORNER_DISTANCE, -CORNER_DISTANCE}, {0, CORNER_DISTANCE, -CORNER_DISTANCE},
                             {0, CORNER_DISTANCE, CORNER_DISTANCE}, {0, -CORNER_DISTANCE, CORNER_DISTANCE}};
    for (int i = lane; i < n; i += RIG_NT) { // first pass: world point, ray direction in the robot frame, camera of every point
        int c = 0;
        while (i >= sBase[c + 1]) c++;
        const int j = i - sBase[c], t = j >> 2, corner = j & 3;
        const ck_iso3_t *tag = a.cam[c].tags + sTagAt[c] + t;
        const double *v = a.cam[c].bearings + 3 * (sBearAt[c] + j);
        double R[9], p[3];
        quat_to_mat(tag->q, R);
        mat3_vec(R, cp[corner], p);
        double *o = pts + (size_t)i * CK_RIG_POINT_DOUBLES;
        for (int k = 0; k < 3; k++) o[k] = p[k] + tag->t[k];
        const double *A = sCamA[c];
        for (int k = 0; k < 3; k++) o[3 + k] = A[k] * v[0] + A[3 + k] * v[1] + A[6 + k] * v[2];
        o[6] = (double)c;
    }
    __syncthreads();
    if (lane < 3) { // centroid over all cameras, index order
        double s = 0;
        for (int i = 0; i < n; i++) s += pts[(size_t)i * CK_RIG_POINT_DOUBLES + lane];
        sCentroid[lane] = s / (double)n;
    }
    __syncthreads();
    // entry e of [Q_rr(81) | Q_rt(27) | Q_tt(9) | q_r(9) | q_t(3) | q_0 | S(6)] belongs to one lane
    for (int e = lane; e < RIG_ENTRIES; e += RIG_NT) {
        double acc = 0;
        for (int k = 0; k < n; k++) {
            const double *pk = pts + (size_t)k * CK_RIG_POINT_DOUBLES, *v = pk + 3;
            double X[3] = {pk[0] - sCentroid[0], pk[1] - sCentroid[1], pk[2] - sCentroid[2]};
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
            } else if (e < 117) {
                int q = e - 108, i = q / 3, j = q - i * 3;
                acc += (i == j ? 1.0 : 0.0) - (v[i] * v[j]) * inv;
            } else if (e >= 130) { // S00 S01 S02 S11 S12 S22
                const int q = e - 130, i = q < 3 ? 0 : (q < 5 ? 1 : 2), j = q < 3 ? q : (q < 5 ? q - 2 : 2);
                acc += X[i] * X[j];
            } else {
                const double *o = sCamO[(int)pk[6]];
                double Mo[3];
#pragma unroll
                for (int i = 0; i < 3; i++)
                    Mo[i] = ((i == 0 ? 1.0 : 0.0) - (v[i] * v[0]) * inv) * o[0] + ((i == 1 ? 1.0 : 0.0) - (v[i] * v[1]) * inv) * o[1] +
                            ((i == 2 ? 1.0 : 0.0) - (v[i] * v[2]) * inv) * o[2];
                if (e < 126) {
                    int row = e - 117, ai = row / 3, i = row - ai * 3;
                    acc += X[ai] * sel3(Mo, i);
                } else if (e < 129) acc += sel3(Mo, e - 126);
                else acc += o[0] * Mo[0] + o[1] * Mo[1] + o[2] * Mo[2];
            }
        }
        if (e < 81) sQrr[e] = acc; else if (e < 108) sQrt[e - 81] = acc; else if (e < 117) sQtt[e - 108] = acc;
        else if (e < 126) sQr[e - 117] = acc; else if (e < 129) sQt[e - 126] = acc; else if (e < 130) sQ0 = acc; else sS[e - 130] = acc;
    }
    __syncthreads();
    if (lane == 0) {
        double inv[9];
        if (!mat3_try_inverse(sQtt, inv)) for (int i = 0; i < 9; i++) inv[i] = 0.0;
        for (int i = 0; i < 9; i++) sQttInv[i] = inv[i];
        // Coplanar points (one tag; tags on one wall) with normal n: R n is free, Omega has the exact null space {vec(a n^T)} and its
        // "three smallest eigenvectors" would be an arbitrary basis of it that says nothing about the pose.  The eigenvectors are then
        // taken on the complement: mu * sum_k v_k v_k^T, v_k = vec(e_k n^T), mu = trace(Q_rr) >= every eigenvalue of Omega, moves
        // that space to the top of the spectrum (sMu = 0: not coplanar).  The refinement keeps Omega itself.
        double S[9] = {sS[0], sS[1], sS[2], sS[1], sS[3], sS[4], sS[2], sS[4], sS[5]}, Sv[9], sw[3];
        jacobi3(S, Sv, sw);
        int k = 0;
        double wmin = sw[0], wmax = sw[0];
        if (sw[1] < wmin) { wmin = sw[1]; k = 1; }
        if (sw[2] < wmin) { wmin = sw[2]; k = 2; }
        if (sw[1] > wmax) wmax = sw[1];
        if (sw[2] > wmax) wmax = sw[2];
        double mu = 0;
        if (wmin <= CK_RIG_PLANAR_EPS * wmax)
            for (int i = 0; i < 9; i++) mu += sQrr[i * 9 + i];
        sMu = mu;
        for (int r = 0; r < 3; r++) { const double row[3] = {Sv[r * 3], Sv[r * 3 + 1], Sv[r * 3 + 2]}; sNrm[r] = sel3(row, k); }
    }
    __syncthreads();
    for (int e = lane; e < 81 + 9 + 1; e += RIG_NT) { // Omega | g | c
        if (e == 90) {
            double w[3];
            mat3_vec(sQttInv, sQt, w);
            sC = sQ0 - (sQt[0] * w[0] + sQt[1] * w[1] + sQt[2] * w[2]);
            continue;
        }
        int i = e < 81 ? e / 9 : e - 81, j = e < 81 ? e - i * 9 : 0;
        double t0 = sQrt[i * 3] * sQttInv[0] + sQrt[i * 3 + 1] * sQttInv[3] + sQrt[i * 3 + 2] * sQttInv[6];
        double t1 = sQrt[i * 3] * sQttInv[1] + sQrt[i * 3 + 1] * sQttInv[4] + sQrt[i * 3 + 2] * sQttInv[7];
        double t2 = sQrt[i * 3] * sQttInv[2] + sQrt[i * 3 + 1] * sQttInv[5] + sQrt[i * 3 + 2] * sQttInv[8];
        if (e < 81) {
            double om = sQrr[e] - (t0 * sQrt[j * 3] + t1 * sQrt[j * 3 + 1] + t2 * sQrt[j * 3 + 2]);
            sOmega[e] = om; sV[e] = (i == j) ? 1.0 : 0.0;
            sA[e] = (sMu != 0.0 && i % 3 == j % 3) ? om + sMu * (sNrm[i / 3] * sNrm[j / 3]) : om;
        } else sG[i] = sQr[i] - (t0 * sQt[0] + t1 * sQt[1] + t2 * sQt[2]);
    }
    __syncthreads();
    jacobi9_wave(sA, sV, lane);
    __syncthreads();
    if (lane == 0) {
        for (int i = 0; i < 9; i++) { sW[i] = sA[i * 9 + i]; sIdx[i] = i; }
        for (int i = 1; i < 9; i++) { // stable ascending order of eigenvalues
            int v = sIdx[i], j = i - 1;
            while (j >= 0 && sW[sIdx[j]] > sW[v]) { sIdx[j + 1] = sIdx[j]; j--; }
            sIdx[j + 1] = v;
        }
        sRot[0] = cos(gyro); sRot[1] = sin(gyro);
    }
    __syncthreads();
    {   // the six starts: group g of 16 lanes = candidate 2*t + sign index
        const int g = lane >> 4, gl = lane & 15;
        if (g < 6) {
            int t = g >> 1;
            double sign = (g & 1) ? 1.0 : -1.0, guess[9], r[9];
            for (int k = 0; k < 9; k++) guess[k] = sV[k * 9 + sIdx[t]] * sign;
            nearest_so3(guess, r);
            double rOr = optimization16<true>(a.prm.sqpnp.max_iter, a.prm.sqpnp.tol_sq, r, sOmega, sG, gl);
            double gr = 0;
            for (int k = 0; k < 9; k++) gr += sG[k] * r[k];
            double energy = (rOr - 2.0 * gr) + sC;
            double dot = r[0] * sRot[0] + r[3] * sRot[1]; // the robot's forward axis in the world is row 0 of R
            double ae = 1.0 - dot;
            if (ae < 0.0) ae = 0.0;
            energy += a.prm.sign_change_error * ae;
            if (gl == 0) {
                for (int k = 0; k < 9; k++) sCandR[g][k] = r[k];
                sCandE[g] = energy;
            }
        }
    }
    __syncthreads();
    if (lane == 0) { // stable sort by penalised energy, in LDS: a runtime-indexed array of a lane's own would live in private memory
        for (int i = 0; i < 6; i++) sOrder[i] = i;
        for (int i = 1; i < 6; i++) {
            int v = sOrder[i], j = i - 1;
            while (j >= 0 && sCandE[sOrder[j]] > sCandE[v]) { sOrder[j + 1] = sOrder[j]; j--; }
            sOrder[j + 1] = v;
        }
    }
    __syncthreads();
    if (lane >= 64) return; // the first wave picks the winner
    bool found = false;
    double best_score = DBLMAX, bestRm[9], bestT[3], best_energy = 0;
    for (int oi = 0; oi < 6; oi++) {
        const double *r = sCandR[sOrder[oi]];
        double Rm[9];
        for (int c = 0; c < 3; c++)
            for (int rr = 0; rr < 3; rr++) Rm[rr * 3 + c] = r[c * 3 + rr];
        double d[3], tl[3], Rc[3], t[3];
        for (int j = 0; j < 3; j++) {
            double s = 0;
            for (int i = 0; i < 9; i++) s += sQrt[i * 3 + j] * r[i];
            d[j] = sQt[j] - s;
        }
        mat3_vec(sQttInv, d, tl);
        mat3_vec(Rm, sCentroid, Rc);
        for (int k = 0; k < 3; k++) t[k] = tl[k] - Rc[k];
        bool behind = false;
        for (int i = lane; i < n; i += 64) {
            const double *pk = pts + (size_t)i * CK_RIG_POINT_DOUBLES;
            const int c = (int)pk[6];
            double pr[3];
            mat3_vec(Rm, pk, pr);
            for (int k = 0; k < 3; k++) pr[k] += t[k];
            if (!((sCamA[c][6] * pr[0] + sCamA[c][7] * pr[1] + sCamA[c][8] * pr[2]) + sCamB[c][2] > 0.0)) behind = true;
        }
        if (__ballot(behind)) continue; // uniform: every point in front of its own camera
        if (sCandE[sOrder[oi]] < best_score) {
            best_score = sCandE[sOrder[oi]];
            for (int k = 0; k < 9; k++) bestRm[k] = Rm[k];
            for (int k = 0; k < 3; k++) bestT[k] = t[k];
            found = true;
        }
    }
    if (!found) return;
    // The pose that is returned: R^ = polar(R), the rotation next to the refinement's last iterate (which meets the constraints to
    // round-off only), and t.  Per camera: its tags and the RMS point-to-ray distance of its own points at that pose.  The squared
    // distances, summed per camera and then over the cameras, are E again, without the cancellation of the quadratic form (terms of
    // the size of |o|^2 * points against a sum of noise^2) and, taken ON the constraint manifold, without the first-order sensitivity
    // to how far off it the iterate ended: that sum is the energy the record and the standard deviations carry.
    double bestR[9];
    polar_rotation(bestRm, bestR);
    double cam_sum = 0;
    if (lane < a.n_cams) {
        const int c = lane, cnt = sCnt[c];
        res->cam_tags[c] = cnt >> 2;
        if (cnt) {
            double s = 0;
            for (int i = sBase[c]; i < sBase[c] + cnt; i++) {
                const double *pk = pts + (size_t)i * CK_RIG_POINT_DOUBLES, *u = pk + 3;
                const double sq = u[0] * u[0] + u[1] * u[1] + u[2] * u[2], inv = 1.0 / sq;
                double d[3], Pd[3];
                mat3_vec(bestR, pk, d);
                for (int k = 0; k < 3; k++) d[k] = (d[k] + bestT[k]) - sCamO[c][k];
                // d^T M d = |M d|^2 (M is a projector): the square of a small vector, not the product of a small with a large one
                const double along = (u[0] * d[0] + u[1] * d[1] + u[2] * d[2]) * inv;
                for (int k = 0; k < 3; k++) Pd[k] = d[k] - u[k] * along;
                s += Pd[0] * Pd[0] + Pd[1] * Pd[1] + Pd[2] * Pd[2];
            }
            res->cam_rms[c] = sqrt((s > 0.0 ? s : 0.0) / (double)cnt);
            cam_sum = s;
        }
    }
    for (int c = 0; c < a.n_cams; c++) best_energy += __shfl(cam_sum, c); // (uniform: the whole first wave is here)
    if (lane != 0) return;
    double distance = sqrt(bestT[0] * bestT[0] + bestT[1] * bestT[1] + bestT[2] * bestT[2]);
    {   // compute_std_devs over all the cameras' tags; a round-off negative energy counts as 0
        double n_points = (double)(n_tags * 4);
        double rms = sqrt((best_energy > 0.0 ? best_energy : 0.0) / n_points);
        if (rms > MAX_TRUSTABLE_RMS) { res->std_devs[0] = res->std_devs[1] = res->std_devs[2] = DBLMAX; }
        else {
            double mult = 1.0 + (distance / TAG_SIZE);
            double xy = ((rms * mult) / sqrt((double)n_tags)) * XY_STD_DEV_SCALAR;
            xy = xy < 0.01 ? 0.01 : (xy > 10.0 ? 10.0 : xy);
            double th = (((rms / TAG_SIZE) * mult) / sqrt((double)n_tags)) * THETA_STD_DEV_SCALAR;
            th = th < 0.05 ? 0.05 : (th > PI_D ? PI_D : th);
            res->std_devs[0] = xy; res->std_devs[1] = xy; res->std_devs[2] = th;
        }
    }
    // world <- robot: rot = polar(R)^T, pos = -rot t; then the yaw pivot about the mean tag centre of all the cameras
    double robot_rot[9], robot_pos[3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) robot_rot[i * 3 + j] = bestR[j * 3 + i];
    for (int k = 0; k < 3; k++) robot_pos[k] = -(robot_rot[k * 3] * bestT[0] + robot_rot[k * 3 + 1] * bestT[1] + robot_rot[k * 3 + 2] * bestT[2]);
    double tc[3] = {0, 0, 0};
    for (int c = 0; c < a.n_cams; c++) {
        const ck_iso3_t *tags = a.cam[c].tags + sTagAt[c];
        for (int t = 0; t < (sCnt[c] >> 2); t++)
            for (int k = 0; k < 3; k++) tc[k] += tags[t].t[k];
    }
    for (int k = 0; k < 3; k++) tc[k] /= (double)n_tags;
    double vision_yaw = atan2(robot_rot[3], robot_rot[0]);
    double delta_yaw = gyro - vision_yaw;
    delta_yaw = fmod(delta_yaw + PI_D, 2.0 * PI_D);
    if (delta_yaw < 0) delta_yaw += 2.0 * PI_D;
    delta_yaw -= PI_D;
    double delta_deg = fabs(delta_yaw) * (180.0 / PI_D);
    double weight = delta_deg / MAX_GYRO_DELTA;
    weight = weight < 0 ? 0 : (weight > 1 ? 1 : weight);
    weight = weight * weight * (3.0 - 2.0 * weight);
    double applied = delta_yaw * weight;
    double cz = cos(applied), sz = sin(applied);
    double rotz[9] = {cz, -sz, 0, sz, cz, 0, 0, 0, 1};
    double rel[3] = {robot_pos[0] - tc[0], robot_pos[1] - tc[1], robot_pos[2] - tc[2]}, piv[3], R2[9];
    mat3_vec(rotz, rel, piv);
    mat3_mul(rotz, robot_rot, R2);
    for (int k = 0; k < 3; k++) res->pos[k] = tc[k] + piv[k];
    for (int k = 0; k < 9; k++) res->rot[k] = R2[k];
    double yaw = 0.0;
    if (fabs(R2[6]) < 1.0) { double pitch = -asin(R2[6]); double tcs = cos(pitch); yaw = atan2(R2[3] / tcs, R2[0] / tcs); }
    res->yaw = yaw;
    res->energy = best_energy;
    res->n_tags = n_tags;
    res->valid = 1;
    if (a.meas) {
        ck_vision_measurement_t m;
        memset(&m, 0, sizeof m);
        m.camera_id = a.prm.rig_id;
        m.pose_x = res->pos[0]; m.pose_y = res->pos[1]; m.pose_rot = yaw;
        m.std_x = res->std_devs[0]; m.std_y = res->std_devs[1]; m.std_rot = res->std_devs[2];
        uint32_t nd = 0; // ALL detections of all the cameras, like the per-camera record's
        for (int c = 0; c < a.n_cams; c++)
            if (a.cam[c].counters) nd += a.cam[c].counters[(size_t)step * CK_CNT_STRIDE + CK_CNT_DETS];
        m.tag_count = (uint8_t)(nd > 255 ? 255 : nd);
        a.meas[step] = m;
        a.valid[step] = 1;
    }
}

// what the kernel needs on the device besides the cameras' arrays: results, gyro, the points of the first pass
static int rig_reserve(ck_rig_ws *ws, int n, int max_points) {
    int rc;
    if ((rc = ws->d_points.reserve(sizeof(double) * CK_RIG_POINT_DOUBLES * (size_t)n * (size_t)(max_points > 0 ? max_points : 1))) != CK_OK) return rc;
    if ((rc = ws->d_res.reserve(sizeof(ck_rig_result_t) * (size_t)n)) != CK_OK) return rc;
    return ws->d_gyro.reserve(sizeof(double) * (size_t)n);
}

} // namespace

extern "C" int ck_rig_solve_batch(ck_handle_t *h, const ck_rig_params_t *params, int32_t n_cams, const ck_sqpnp_problem_t *problems, int32_t n,
                                  const ck_iso3_t *tags, int32_t n_tags_total, const double *bearings, int32_t n_bearings_total,
                                  const double *gyro, ck_rig_result_t *out) {
    if (!h || !params || !problems || n < 0 || n_cams < 1 || n_cams > CK_RIG_MAX_CAMS) return CK_EINVAL;
    if (n == 0) return ck_rig_check(params, n_cams, problems, 0, tags, n_tags_total, bearings, n_bearings_total, gyro, out, nullptr);
    CK_HIP(hipSetDevice(h->device));
    // the records may lie on the device: the checks read a host copy
    std::vector<ck_sqpnp_problem_t> rec((size_t)n_cams * (size_t)n);
    CK_HIP(hipMemcpy(rec.data(), problems, sizeof(ck_sqpnp_problem_t) * rec.size(), hipMemcpyDefault));
    int32_t max_points = 0;
    int rc = ck_rig_check(params, n_cams, rec.data(), n, tags, n_tags_total, bearings, n_bearings_total, gyro, out, &max_points);
    if (rc != CK_OK) return rc;
    ck_rig_ws *ws = ck_workspace(h->rig);
    if (!ws) return CK_ENOMEM;
    if ((rc = rig_reserve(ws, n, max_points)) != CK_OK) return rc;
    if ((rc = ws->d_prob.reserve(sizeof(ck_sqpnp_problem_t) * rec.size())) != CK_OK) return rc;
    if ((rc = ws->d_tags.reserve(sizeof(ck_iso3_t) * (size_t)(n_tags_total ? n_tags_total : 1))) != CK_OK) return rc;
    if ((rc = ws->d_bearings.reserve(sizeof(double) * 3 * (size_t)(n_bearings_total ? n_bearings_total : 1))) != CK_OK) return rc;
    CK_HIP(hipMemcpyAsync(ws->d_prob, rec.data(), sizeof(ck_sqpnp_problem_t) * rec.size(), hipMemcpyHostToDevice, h->stream));
    if (n_tags_total) CK_HIP(hipMemcpyAsync(ws->d_tags, tags, sizeof(ck_iso3_t) * (size_t)n_tags_total, hipMemcpyDefault, h->stream));
    if (n_bearings_total) CK_HIP(hipMemcpyAsync(ws->d_bearings, bearings, sizeof(double) * 3 * (size_t)n_bearings_total, hipMemcpyDefault, h->stream));
    CK_HIP(hipMemcpyAsync(ws->d_gyro, gyro, sizeof(double) * (size_t)n, hipMemcpyDefault, h->stream));
    RigArgs a;
    memset(&a, 0, sizeof a);
    a.prm = *params;
    for (int c = 0; c < n_cams; c++) a.cam[c] = {ws->d_prob.p + (size_t)c * n, ws->d_tags, ws->d_bearings, nullptr, 0, 0};
    a.n_cams = n_cams; a.n = n; a.max_points = max_points;
    a.gyro = ws->d_gyro; a.points = ws->d_points; a.out = ws->d_res;
    hipLaunchKernelGGL(k_rig, dim3((unsigned)n), dim3(RIG_NT), 0, h->stream, a);
    CK_HIP(hipGetLastError());
    CK_HIP(hipMemcpyAsync(out, ws->d_res, sizeof(ck_rig_result_t) * (size_t)n, hipMemcpyDefault, h->stream));
    CK_HIP(hipStreamSynchronize(h->stream)); // (rec, a pageable source of the first copy, lives until here)
    return CK_OK;
}

// ck_rig_process_last up to, not including, the wait for the stream
static int rig_enqueue_last(ck_handle_t *const *handles, int32_t n_cams, int32_t n, const ck_rig_params_t *params, const double *gyro,
                            const uint8_t *has_gyro, ck_rig_result_t *out, ck_vision_measurement_t *meas, int32_t *valid) {
    if (!handles || !params || !gyro || !has_gyro || !meas || !valid || n_cams < 1 || n_cams > CK_RIG_MAX_CAMS || n < 1) return CK_EINVAL;
    for (int c = 0; c < n_cams; c++) {
        const ck_handle *hc = handles[c];
        // n_pose_inputs: the glue records and the detection counts of a ck_process_* call are still the workspace's
        if (!hc || hc->device != handles[0]->device || hc->n_last_pose != n || hc->n_pose_inputs != n) return CK_EINVAL;
    }
    ck_handle *h = handles[0];
    CK_HIP(hipSetDevice(h->device));
    ck_rig_ws *ws = ck_workspace(h->rig);
    if (!ws) return CK_ENOMEM;
    int max_points = 0; // what the cameras can hold, not what they saw: the counts lie on the device, and reading them would cost a round trip
    for (int c = 0; c < n_cams; c++) max_points += 4 * handles[c]->ws.det_cap;
    int rc = rig_reserve(ws, n, max_points);
    if (rc != CK_OK) return rc;
    if ((rc = ws->d_has_gyro.reserve((size_t)n)) != CK_OK) return rc;
    if ((rc = ws->d_meas.reserve(sizeof(ck_vision_measurement_t) * (size_t)n)) != CK_OK) return rc;
    if ((rc = ws->d_valid.reserve(sizeof(int32_t) * (size_t)n)) != CK_OK) return rc;
    for (int c = 1; c < n_cams; c++) { // the other cameras' records are complete before the kernel reads them in place
        if (!ws->ev[c]) CK_HIP_ALLOC(hipEventCreateWithFlags(&ws->ev[c], hipEventDisableTiming));
        CK_HIP(hipEventRecord(ws->ev[c], handles[c]->stream));
        CK_HIP(hipStreamWaitEvent(h->stream, ws->ev[c], 0));
    }
    CK_HIP(hipMemcpyAsync(ws->d_gyro, gyro, sizeof(double) * (size_t)n, hipMemcpyDefault, h->stream));
    CK_HIP(hipMemcpyAsync(ws->d_has_gyro, has_gyro, (size_t)n, hipMemcpyDefault, h->stream));
    RigArgs a;
    memset(&a, 0, sizeof a);
    a.prm = *params;
    for (int c = 0; c < n_cams; c++) {
        const ck_stage_ws &w = handles[c]->ws;
        a.cam[c] = {w.d_problems, w.d_pose_tags, w.d_bearings, w.d_counters, w.det_cap, 0};
    }
    a.n_cams = n_cams; a.n = n; a.max_points = max_points;
    a.gyro = ws->d_gyro; a.has_gyro = ws->d_has_gyro; a.points = ws->d_points; a.out = ws->d_res;
    a.meas = ws->d_meas; a.valid = ws->d_valid;
    hipLaunchKernelGGL(k_rig, dim3((unsigned)n), dim3(RIG_NT), 0, h->stream, a);
    CK_HIP(hipGetLastError());
    if (out) CK_HIP(hipMemcpyAsync(out, ws->d_res, sizeof(ck_rig_result_t) * (size_t)n, hipMemcpyDefault, h->stream));
    CK_HIP(hipMemcpyAsync(meas, ws->d_meas, sizeof(ck_vision_measurement_t) * (size_t)n, hipMemcpyDefault, h->stream));
    CK_HIP(hipMemcpyAsync(valid, ws->d_valid, sizeof(int32_t) * (size_t)n, hipMemcpyDefault, h->stream));
    return CK_OK;
}

extern "C" int ck_rig_process_last(ck_handle_t *const *handles, int32_t n_cams, int32_t n, const ck_rig_params_t *params, const double *gyro,
                                   const uint8_t *has_gyro, ck_rig_result_t *out, ck_vision_measurement_t *meas, int32_t *valid) {
    const int rc = rig_enqueue_last(handles, n_cams, n, params, gyro, has_gyro, out, meas, valid);
    if (rc != CK_OK) return rc;
    CK_HIP(hipStreamSynchronize(handles[0]->stream));
    return CK_OK;
}

extern "C" int ck_rig_time_last(ck_handle_t *const *handles, int32_t n_cams, int32_t n, const ck_rig_params_t *params, const double *gyro,
                                const uint8_t *has_gyro, int32_t iters, float *ms_rig, float *ms_sqpnp) {
    if (iters < 1 || !ms_rig || !ms_sqpnp || n < 1) return CK_EINVAL;
    std::vector<ck_vision_measurement_t> meas((size_t)n);
    std::vector<int32_t> valid((size_t)n);
    int rc = rig_enqueue_last(handles, n_cams, n, params, gyro, has_gyro, nullptr, meas.data(), valid.data()); // (checks, workspace)
    if (rc != CK_OK) return rc;
    ck_handle *h = handles[0];
    CK_HIP(hipStreamSynchronize(h->stream));
    hipEvent_t e0, e1;
    CK_HIP_ALLOC(hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); (void)hipGetLastError(); return CK_ENOMEM; }
    for (int it = 0; it < iters && rc == CK_OK; it++) {
        float *dst[2] = {ms_rig + it, ms_sqpnp + it};
        for (int which = 0; which < 2 && rc == CK_OK; which++) {
            if (hipEventRecord(e0, h->stream) != hipSuccess) { rc = CK_EDEVICE; break; }
            if (which == 0) rc = rig_enqueue_last(handles, n_cams, n, params, gyro, has_gyro, nullptr, meas.data(), valid.data());
            else for (int c = 0; c < n_cams && rc == CK_OK; c++) rc = ck_launch_sqpnp_last(handles[c], n, &params->sqpnp, h->stream);
            if (rc != CK_OK) break;
            if (hipEventRecord(e1, h->stream) != hipSuccess || hipEventSynchronize(e1) != hipSuccess ||
                hipEventElapsedTime(dst[which], e0, e1) != hipSuccess) rc = CK_EDEVICE;
        }
    }
    (void)hipStreamSynchronize(h->stream);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (rc == CK_EDEVICE) (void)hipGetLastError();
    return rc;
}
