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
#include "ck_rig.h"
#include "ck_sqpnp_dev.h"

namespace {

struct RigCam {
    const ck_sqpnp_problem_t *problems; // [n] this camera's record of every step
    const ck_iso3_t *tags;
    const double *bearings;
    const uint32_t *counters;           // the handle's per-frame counters (detections for tag_count), or null
    int det_cap;                        // > 0: a handle's workspace, step s owns tags[s * det_cap ..] and bearings[s * det_cap * 4 ..] (what
                                        // k_glue wrote into the records' offsets too: they are not read); 0: the records' offsets
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

struct RigRobustArgs {
    RigArgs a;                          // a.out is not used: the record's `fused` takes its place
    double gate_rad, mu_factor;
    int max_rounds, min_inlier_tags;
    ck_rig_robust_result_t *out;        // [n]
};

constexpr int RIG_NT = 128;
constexpr int RIG_ENTRIES = 117 + 13 + 6; // Q_rr(81) | Q_rt(27) | Q_tt(9) | q_r(9) | q_t(3) | q_0 | scatter of the centred points (6)
constexpr int RIG_ROBUST_TAGS = CK_RIG_MAX_CAMS * CK_RIG_ROBUST_MAX_TAGS;

// The solve of one step is a sequence of pieces over this LDS state, and the two kernels are two ways through them: k_rig once, k_rig_robust
//  once on all tags, once per GNC round with one start, once more on the inliers.  RB = false compiles the tag weights
// out (k_rig); with RB = true `wt` holds one weight per tag (the tags numbered camera-major, then by the record's index: tag of point
// k = k >> 2), a point of weight 0 is skipped and every other contribution is multiplied by its weight: exact for a weight of 1, so
// a pass over weights of 0 and 1 is, bit for bit, the plain pass over the input without the tags of weight 0.  `weighted` false (a step of
// more tags than the weights have room for) counts every tag once.
struct RigLds {
    double sQrr[81], sQrt[27], sQtt[9], sQttInv[9], sOmega[81], sA[81], sV[81], sW[9];
    double sQr[9], sQt[3], sQ0, sG[9], sC, sS[6], sNrm[3], sMu;
    double sCandR[6][9], sCandE[6];
    double sCentroid[3], sRot[2];
    double sCamA[CK_RIG_MAX_CAMS][9], sCamB[CK_RIG_MAX_CAMS][3], sCamO[CK_RIG_MAX_CAMS][3];
    long long sTagAt[CK_RIG_MAX_CAMS], sBearAt[CK_RIG_MAX_CAMS];
    int sCnt[CK_RIG_MAX_CAMS], sBase[CK_RIG_MAX_CAMS + 1], sIdx[9], sOrder[6];
};

template <bool RB>
static __device__ __forceinline__ double rig_weight(const double *wt, bool weighted, int point) {
    if constexpr (RB) return weighted ? wt[point >> 2] : 1.0;
    else return 1.0;
}

// one lane per camera: its mount, its ray origin, its points of this step; then the cameras' first points.  Ends behind a barrier.
static __device__ __forceinline__ void rig_setup(const RigArgs &a, RigLds &L, int step, int lane) {
    if (lane < CK_RIG_MAX_CAMS) {
        const int c = lane;
        int cnt = 0;
        if (c < a.n_cams) {
            const ck_sqpnp_problem_t *p = &a.cam[c].problems[step];
            const int nt = p->n_tags, cap = a.cam[c].det_cap;
            if (nt > 0 && (cap == 0 || nt <= cap)) cnt = 4 * nt;
            L.sTagAt[c] = cap > 0 ? (long long)step * cap : (long long)p->tag_offset;
            L.sBearAt[c] = cap > 0 ? (long long)step * cap * 4 : (long long)p->bearing_offset;
            double A[9], o[3];
            quat_to_mat(p->robot_to_cam.q, A);
            const double b[3] = {p->robot_to_cam.t[0], p->robot_to_cam.t[1], p->robot_to_cam.t[2]};
            ckp_camera_origin(A, b, o);
            for (int k = 0; k < 9; k++) L.sCamA[c][k] = A[k];
            for (int k = 0; k < 3; k++) {
                L.sCamB[c][k] = b[k];
                L.sCamO[c][k] = o[k];
            }
        }
        L.sCnt[c] = cnt;
    }
    __syncthreads();
    if (lane == 0) {
        int s = 0;
        for (int c = 0; c < CK_RIG_MAX_CAMS; c++) { L.sBase[c] = s; s += L.sCnt[c]; }
        L.sBase[CK_RIG_MAX_CAMS] = s;
    }
    __syncthreads();
}

// first pass: world point, ray direction in the robot frame, camera of every point
static __device__ __forceinline__ void rig_first_pass(const RigArgs &a, RigLds &L, double *pts, int n, int lane) {
    for (int i = lane; i < n; i += RIG_NT) {
        int c = 0;
        while (i >= L.sBase[c + 1]) c++;
        const int j = i - L.sBase[c], t = j >> 2, corner = j & 3;
        const ck_iso3_t *tag = a.cam[c].tags + L.sTagAt[c] + t;
        const double *v = a.cam[c].bearings + 3 * (L.sBearAt[c] + j);
        double R[9];
        quat_to_mat(tag->q, R);
        double *o = pts + (size_t)i * CK_RIG_POINT_DOUBLES;
        ckp_tag_corner(R, tag->t, corner, o);
        ckp_ray(L.sCamA[c], v, o + 3);
        o[6] = (double)c;
    }
}

// the (weighted) centroid and the accumulated entries.  Starts and ends behind a barrier of the caller's.
template <bool RB>
static __device__ __forceinline__ void rig_accumulate(RigLds &L, const double *pts, int n, const double *wt, bool weighted, int lane) {
    if (lane < 3) { // centroid over all cameras, index order
        double s = 0;
        if constexpr (RB) {
            double sw = 0;
            for (int i = 0; i < n; i++) {
                const double w = rig_weight<RB>(wt, weighted, i);
                if (w == 0.0) continue;
                s += w * pts[(size_t)i * CK_RIG_POINT_DOUBLES + lane];
                sw += w;
            }
            L.sCentroid[lane] = s / sw;
        } else {
            for (int i = 0; i < n; i++) s += pts[(size_t)i * CK_RIG_POINT_DOUBLES + lane];
            L.sCentroid[lane] = s / (double)n;
        }
    }
    __syncthreads();
    // entry e of [Q_rr(81) | Q_rt(27) | Q_tt(9) | q_r(9) | q_t(3) | q_0 | S(6)] belongs to one lane
    for (int e = lane; e < RIG_ENTRIES; e += RIG_NT) {
        double acc = 0;
        for (int k = 0; k < n; k++) {
            const double w = rig_weight<RB>(wt, weighted, k);
            if (RB && w == 0.0) continue;
            const double *pk = pts + (size_t)k * CK_RIG_POINT_DOUBLES, *v = pk + 3;
            double X[3] = {pk[0] - L.sCentroid[0], pk[1] - L.sCentroid[1], pk[2] - L.sCentroid[2]};
            double sq = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
            double inv = 1.0 / sq;
            double term;
            if (e < 81) {
                int row = e / 9, col = e - row * 9;
                int ai = row / 3, i = row - ai * 3, bi = col / 3, j = col - bi * 3;
                double P = (i == j ? 1.0 : 0.0) - (v[i] * v[j]) * inv;
                term = (P * X[ai]) * X[bi];
            } else if (e < 108) {
                int q = e - 81, row = q / 3, j = q - row * 3;
                int ai = row / 3, i = row - ai * 3;
                double P = (i == j ? 1.0 : 0.0) - (v[i] * v[j]) * inv;
                term = P * X[ai];
            } else if (e < 117) {
                int q = e - 108, i = q / 3, j = q - i * 3;
                term = (i == j ? 1.0 : 0.0) - (v[i] * v[j]) * inv;
            } else if (e >= 130) { // S00 S01 S02 S11 S12 S22
                const int q = e - 130, i = q < 3 ? 0 : (q < 5 ? 1 : 2), j = q < 3 ? q : (q < 5 ? q - 2 : 2);
                term = X[i] * X[j];
            } else {
                const double *o = L.sCamO[(int)pk[6]];
                double Mo[3];
#pragma unroll
                for (int i = 0; i < 3; i++)
                    Mo[i] = ((i == 0 ? 1.0 : 0.0) - (v[i] * v[0]) * inv) * o[0] + ((i == 1 ? 1.0 : 0.0) - (v[i] * v[1]) * inv) * o[1] +
                            ((i == 2 ? 1.0 : 0.0) - (v[i] * v[2]) * inv) * o[2];
                if (e < 126) {
                    int row = e - 117, ai = row / 3, i = row - ai * 3;
                    term = X[ai] * sel3(Mo, i);
                } else if (e < 129) term = sel3(Mo, e - 126);
                else term = o[0] * Mo[0] + o[1] * Mo[1] + o[2] * Mo[2];
            }
            if constexpr (RB) acc += w * term; else acc += term;
        }
        if (e < 81) L.sQrr[e] = acc; else if (e < 108) L.sQrt[e - 81] = acc; else if (e < 117) L.sQtt[e - 108] = acc;
        else if (e < 126) L.sQr[e - 117] = acc; else if (e < 129) L.sQt[e - 126] = acc; else if (e < 130) L.sQ0 = acc; else L.sS[e - 130] = acc;
    }
}

// Q_tt^-1, Omega | g | c and, with `starts`, what the six starts need beside them (the coplanar test; sA and sV for the Jacobi).
// Starts and ends behind a barrier.
static __device__ __forceinline__ void rig_reduce(RigLds &L, bool starts, int lane) {
    __syncthreads();
    if (lane == 0) {
        double inv[9];
        if (!mat3_try_inverse(L.sQtt, inv)) for (int i = 0; i < 9; i++) inv[i] = 0.0;
        for (int i = 0; i < 9; i++) L.sQttInv[i] = inv[i];
        // Coplanar points (one tag; tags on one wall) with normal n: R n is free, Omega has the exact null space {vec(a n^T)} and its
        // "three smallest eigenvectors" would be an arbitrary basis of it that says nothing about the pose.  The eigenvectors are then
        // taken on the complement: mu * sum_k v_k v_k^T, v_k = vec(e_k n^T), mu = trace(Q_rr) >= every eigenvalue of Omega, moves
        // that space to the top of the spectrum (sMu = 0: not coplanar).  The refinement keeps Omega itself.
        double mu = 0;
        if (starts) {
            double S[9] = {L.sS[0], L.sS[1], L.sS[2], L.sS[1], L.sS[3], L.sS[4], L.sS[2], L.sS[4], L.sS[5]}, Sv[9], sw[3];
            jacobi3(S, Sv, sw);
            int k = 0;
            double wmin = sw[0], wmax = sw[0];
            if (sw[1] < wmin) { wmin = sw[1]; k = 1; }
            if (sw[2] < wmin) { wmin = sw[2]; k = 2; }
            if (sw[1] > wmax) wmax = sw[1];
            if (sw[2] > wmax) wmax = sw[2];
            if (wmin <= CK_RIG_PLANAR_EPS * wmax)
                for (int i = 0; i < 9; i++) mu += L.sQrr[i * 9 + i];
            for (int r = 0; r < 3; r++) { const double row[3] = {Sv[r * 3], Sv[r * 3 + 1], Sv[r * 3 + 2]}; L.sNrm[r] = sel3(row, k); }
        }
        L.sMu = mu;
    }
    __syncthreads();
    for (int e = lane; e < 81 + 9 + 1; e += RIG_NT) { // Omega | g | c
        if (e == 90) {
            double w[3];
            mat3_vec(L.sQttInv, L.sQt, w);
            L.sC = L.sQ0 - (L.sQt[0] * w[0] + L.sQt[1] * w[1] + L.sQt[2] * w[2]);
            continue;
        }
        int i = e < 81 ? e / 9 : e - 81, j = e < 81 ? e - i * 9 : 0;
        double t0 = L.sQrt[i * 3] * L.sQttInv[0] + L.sQrt[i * 3 + 1] * L.sQttInv[3] + L.sQrt[i * 3 + 2] * L.sQttInv[6];
        double t1 = L.sQrt[i * 3] * L.sQttInv[1] + L.sQrt[i * 3 + 1] * L.sQttInv[4] + L.sQrt[i * 3 + 2] * L.sQttInv[7];
        double t2 = L.sQrt[i * 3] * L.sQttInv[2] + L.sQrt[i * 3 + 1] * L.sQttInv[5] + L.sQrt[i * 3 + 2] * L.sQttInv[8];
        if (e < 81) {
            double om = L.sQrr[e] - (t0 * L.sQrt[j * 3] + t1 * L.sQrt[j * 3 + 1] + t2 * L.sQrt[j * 3 + 2]);
            L.sOmega[e] = om; L.sV[e] = (i == j) ? 1.0 : 0.0;
            L.sA[e] = (L.sMu != 0.0 && i % 3 == j % 3) ? om + L.sMu * (L.sNrm[i / 3] * L.sNrm[j / 3]) : om;
        } else L.sG[i] = L.sQr[i] - (t0 * L.sQt[0] + t1 * L.sQt[1] + t2 * L.sQt[2]);
    }
    __syncthreads();
}

// the six refined starts in sCandR / sCandE and their order by penalised energy in sOrder.  Starts and ends behind a barrier.
static __device__ __forceinline__ void rig_six_starts(const ck_rig_params_t &prm, RigLds &L, double gyro, int lane) {
    jacobi9_wave(L.sA, L.sV, lane);
    __syncthreads();
    if (lane == 0) {
        for (int i = 0; i < 9; i++) { L.sW[i] = L.sA[i * 9 + i]; L.sIdx[i] = i; }
        for (int i = 1; i < 9; i++) { // stable ascending order of eigenvalues
            int v = L.sIdx[i], j = i - 1;
            while (j >= 0 && L.sW[L.sIdx[j]] > L.sW[v]) { L.sIdx[j + 1] = L.sIdx[j]; j--; }
            L.sIdx[j + 1] = v;
        }
        L.sRot[0] = cos(gyro); L.sRot[1] = sin(gyro);
    }
    __syncthreads();
    {   // the six starts: group g of 16 lanes = candidate 2*t + sign index
        const int g = lane >> 4, gl = lane & 15;
        if (g < 6) {
            int t = g >> 1;
            double sign = (g & 1) ? 1.0 : -1.0, guess[9], r[9];
            for (int k = 0; k < 9; k++) guess[k] = L.sV[k * 9 + L.sIdx[t]] * sign;
            // (k_rig_robust calls both of these from a second place; left to itself the compiler then inlines neither, and r[9] would
            // go through private memory)
            [[clang::always_inline]] nearest_so3(guess, r);
            double rOr;
            [[clang::always_inline]] rOr = optimization16<true>(prm.sqpnp.max_iter, prm.sqpnp.tol_sq, r, L.sOmega, L.sG, gl);
            double gr = 0;
            for (int k = 0; k < 9; k++) gr += L.sG[k] * r[k];
            double energy = (rOr - 2.0 * gr) + L.sC;
            double dot = r[0] * L.sRot[0] + r[3] * L.sRot[1]; // the robot's forward axis in the world is row 0 of R
            double ae = 1.0 - dot;
            if (ae < 0.0) ae = 0.0;
            energy += prm.sign_change_error * ae;
            if (gl == 0) {
                for (int k = 0; k < 9; k++) L.sCandR[g][k] = r[k];
                L.sCandE[g] = energy;
            }
        }
    }
    __syncthreads();
    if (lane == 0) { // stable sort by penalised energy, in LDS: a runtime-indexed array of a lane's own would live in private memory
        for (int i = 0; i < 6; i++) L.sOrder[i] = i;
        for (int i = 1; i < 6; i++) {
            int v = L.sOrder[i], j = i - 1;
            while (j >= 0 && L.sCandE[L.sOrder[j]] > L.sCandE[v]) { L.sOrder[j + 1] = L.sOrder[j]; j--; }
            L.sOrder[j + 1] = v;
        }
    }
    __syncthreads();
}

// R (row-major) of r (column-major) and the t that goes with it
static __device__ __forceinline__ void rig_translation(const RigLds &L, const double *r, double Rm[9], double t[3]) {
    ckp_translation(L.sQrt, L.sQt, L.sQttInv, L.sCentroid, r, Rm, t);
}

// The whole first wave: the cheapest candidate with every point (of a weight other than 0) in front of its own camera.
template <bool RB>
static __device__ __forceinline__ bool rig_pick(const RigLds &L, const double *pts, int n, const double *wt, bool weighted, int lane, double bestRm[9],
                                                double bestT[3]) {
    bool found = false;
    double best_score = DBL_MAX;
    for (int oi = 0; oi < 6; oi++) {
        double Rm[9], t[3];
        rig_translation(L, L.sCandR[L.sOrder[oi]], Rm, t);
        bool behind = false;
        for (int i = lane; i < n; i += 64) {
            if (RB && rig_weight<RB>(wt, weighted, i) == 0.0) continue;
            const double *pk = pts + (size_t)i * CK_RIG_POINT_DOUBLES;
            const int c = (int)pk[6];
            double pr[3];
            mat3_vec(Rm, pk, pr);
            for (int k = 0; k < 3; k++) pr[k] += t[k];
            if (!((L.sCamA[c][6] * pr[0] + L.sCamA[c][7] * pr[1] + L.sCamA[c][8] * pr[2]) + L.sCamB[c][2] > 0.0)) behind = true;
        }
        if (__ballot(behind)) continue; // uniform: every point in front of its own camera
        if (L.sCandE[L.sOrder[oi]] < best_score) {
            best_score = L.sCandE[L.sOrder[oi]];
            for (int k = 0; k < 9; k++) bestRm[k] = Rm[k];
            for (int k = 0; k < 3; k++) bestT[k] = t[k];
            found = true;
        }
    }
    return found;
}

// The whole first wave: the record (and the measurement) of the chosen candidate.  bestR = polar(bestRm) comes back in every lane.
template <bool RB>
static __device__ __forceinline__ void rig_finish(const RigArgs &a, const RigLds &L, const double *pts, const double *wt, bool weighted, int step, int lane,
                                                  double gyro, const double bestRm[9], const double bestT[3], double bestR[9],
                                                  ck_rig_result_t *res) {
    // The pose that is returned: R^ = polar(R), the rotation next to the refinement's last iterate (which meets the constraints to
    // round-off only), and t.  Per camera: its tags and the RMS point-to-ray distance of its own points at that pose.  The squared
    // distances, summed per camera and then over the cameras, are E again, without the cancellation of the quadratic form (terms of
    // the size of |o|^2 * points against a sum of noise^2) and, taken ON the constraint manifold, without the first-order sensitivity
    // to how far off it the iterate ended: that sum is the energy the record and the standard deviations carry.
    polar_rotation(bestRm, bestR);
    double cam_sum = 0, best_energy = 0;
    int cam_n = 0, n_tags = 0;
    if (lane < a.n_cams) {
        const int c = lane;
        int cnt = L.sCnt[c];
        if constexpr (RB) {
            cnt = 0;
            for (int i = L.sBase[c]; i < L.sBase[c] + L.sCnt[c]; i += 4)
                if (rig_weight<RB>(wt, weighted, i) != 0.0) cnt += 4;
        }
        res->cam_tags[c] = cnt >> 2;
        cam_n = cnt >> 2;
        if (cnt) {
            double s = 0;
            for (int i = L.sBase[c]; i < L.sBase[c] + L.sCnt[c]; i++) {
                if (RB && rig_weight<RB>(wt, weighted, i) == 0.0) continue;
                const double *pk = pts + (size_t)i * CK_RIG_POINT_DOUBLES;
                double ud, dd;
                s += ckp_ray_residual(bestR, bestT, pk, pk + 3, L.sCamO[c], &ud, &dd);
            }
            res->cam_rms[c] = sqrt((s > 0.0 ? s : 0.0) / (double)cnt);
            cam_sum = s;
        }
    }
    for (int c = 0; c < a.n_cams; c++) { // (uniform: the whole first wave is here)
        best_energy += __shfl(cam_sum, c);
        n_tags += __shfl(cam_n, c);
    }
    if (lane != 0) return;
    double distance = sqrt(bestT[0] * bestT[0] + bestT[1] * bestT[1] + bestT[2] * bestT[2]);
    // over all the cameras' tags; a round-off negative energy counts as 0
    ckp_std_devs(best_energy > 0.0 ? best_energy : 0.0, n_tags, distance, res->std_devs);
    // world <- robot: rot = polar(R)^T, pos = -rot t; then the yaw pivot about the mean tag centre of all the cameras
    double robot_rot[9], robot_pos[3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) robot_rot[i * 3 + j] = bestR[j * 3 + i];
    for (int k = 0; k < 3; k++) robot_pos[k] = -(robot_rot[k * 3] * bestT[0] + robot_rot[k * 3 + 1] * bestT[1] + robot_rot[k * 3 + 2] * bestT[2]);
    double tc[3] = {0, 0, 0};
    for (int c = 0; c < a.n_cams; c++) {
        const ck_iso3_t *tags = a.cam[c].tags + L.sTagAt[c];
        for (int t = 0; t < (L.sCnt[c] >> 2); t++) {
            if (RB && rig_weight<RB>(wt, weighted, L.sBase[c] + 4 * t) == 0.0) continue;
            for (int k = 0; k < 3; k++) tc[k] += tags[t].t[k];
        }
    }
    for (int k = 0; k < 3; k++) tc[k] /= (double)n_tags;
    double yaw;
    ckp_yaw_pivot(robot_rot, robot_pos, tc, gyro, res->rot, res->pos, &yaw);
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

// the heartbeat measurement of a step without a pose
static __device__ __forceinline__ void rig_blank_meas(const RigArgs &a, int step) {
    ck_vision_measurement_t m;
    memset(&m, 0, sizeof m);
    m.camera_id = a.prm.rig_id;
    a.meas[step] = m;
    a.valid[step] = 0;
}

__global__ __launch_bounds__(RIG_NT) void k_rig(RigArgs a) {
    __shared__ RigLds L;
    const int lane = threadIdx.x, step = blockIdx.x;
    if (step >= a.n) return;
    ck_rig_result_t *res = &a.out[step];
    // the record of a step without a pose: all zero (and the heartbeat measurement).  The first wave writes it and lane 0 of the same
    // wave the pose at the end, so the stores to one address stay in order
    if (lane < (int)(sizeof(ck_rig_result_t) / 4)) reinterpret_cast<uint32_t *>(res)[lane] = 0u;
    if (lane == 0 && a.meas) rig_blank_meas(a, step);
    rig_setup(a, L, step, lane);
    const int n = L.sBase[CK_RIG_MAX_CAMS];
    const bool has_gyro = a.has_gyro ? a.has_gyro[step] != 0 : true;
    if (n < 3 || n > a.max_points || !has_gyro) return; // uniform: no tag in any camera, or "no gyro, no solve"
    const double gyro = a.gyro[step];
    double *pts = a.points + (size_t)step * a.max_points * CK_RIG_POINT_DOUBLES;
    rig_first_pass(a, L, pts, n, lane);
    __syncthreads();
    rig_accumulate<false>(L, pts, n, nullptr, false, lane);
    rig_reduce(L, true, lane);
    rig_six_starts(a.prm, L, gyro, lane);
    if (lane >= 64) return; // the first wave picks the winner
    double bestRm[9], bestT[3], bestR[9];
    if (!rig_pick<false>(L, pts, n, nullptr, false, lane, bestRm, bestT)) return;
    rig_finish<false>(a, L, pts, nullptr, false, step, lane, gyro, bestRm, bestT, bestR, res);
}

// ---- the robust solve (chalkydri_hip.h has the arithmetic, ck_rig_host.c: solve_step_robust is the same on the host) ----
struct RigRobustLds {
    double rho[RIG_ROBUST_TAGS], wt[RIG_ROBUST_TAGS]; // per tag, 8 KB
    double Rm[9], T[3];                               // the pose the residuals are taken at: R row-major
    double r[9];                                      // ... and its r (column-major), the next round's start
    double rho_max;
    int found, verdict, n_in;
};
// rho of the tags j = first, first + stride, ... at (R row-major, t): the mean over the four corners of e^2
static __device__ __forceinline__ void rig_tag_rho(const RigLds &L, const double *pts, int n_tags, const double *R, const double *t,
                                                   double *rho, int first, int stride) {
    for (int j = first; j < n_tags; j += stride) {
        double s = 0;
        for (int i = 4 * j; i < 4 * j + 4; i++) {
            const double *pk = pts + (size_t)i * CK_RIG_POINT_DOUBLES;
            double ud, dd;
            const double pp = ckp_ray_residual(R, t, pk, pk + 3, L.sCamO[(int)pk[6]], &ud, &dd);
            s += (ud > 0.0 && dd > 0.0) ? pp / dd : 1.0;
        }
        rho[j] = s * 0.25;
    }
}

__global__ __launch_bounds__(RIG_NT) void k_rig_robust(RigRobustArgs ra) {
    __shared__ RigLds L;
    __shared__ RigRobustLds B;
    const RigArgs &a = ra.a;
    const int lane = threadIdx.x, step = blockIdx.x;
    if (step >= a.n) return;
    ck_rig_robust_result_t *out = &ra.out[step];
    // every store to the record is the first wave's, in program order: the zeroes here, what lane 0 and the cameras' lanes know later
    if (lane < 64)
        for (int k = lane; k < (int)(sizeof(ck_rig_robust_result_t) / 4); k += 64) reinterpret_cast<uint32_t *>(out)[k] = 0u;
    if (lane == 0 && a.meas) rig_blank_meas(a, step);
    rig_setup(a, L, step, lane);
    const int n = L.sBase[CK_RIG_MAX_CAMS], n_tags = n >> 2;
    const bool has_gyro = a.has_gyro ? a.has_gyro[step] != 0 : true;
    if (n < 3 || n > a.max_points || !has_gyro) return; // uniform
    // a camera with more tags than a mask has bits (only a handle's workspace can bring one: the stand-alone call refuses it): the
    // plain solve, no weights
    bool plain_only = false;
    for (int c = 0; c < CK_RIG_MAX_CAMS; c++) plain_only |= L.sCnt[c] > 4 * CK_RIG_ROBUST_MAX_TAGS;
    const bool weighted = !plain_only;
    const double gyro = a.gyro[step], c = ra.gate_rad, c2 = c * c;
    double *pts = a.points + (size_t)step * a.max_points * CK_RIG_POINT_DOUBLES;
    rig_first_pass(a, L, pts, n, lane);
    if (!plain_only)
        for (int j = lane; j < n_tags; j += RIG_NT) B.wt[j] = 1.0;
    __syncthreads();
    int rounds = 0;
    bool maxed = false;
    for (bool final_pass = false;; final_pass = true) { // at most twice: all the tags, then the inliers
        rig_accumulate<true>(L, pts, n, B.wt, weighted, lane);
        rig_reduce(L, true, lane);
        rig_six_starts(a.prm, L, gyro, lane);
        if (lane < 64) {
            double bestRm[9], bestT[3];
            const bool found = rig_pick<true>(L, pts, n, B.wt, weighted, lane, bestRm, bestT);
            if (!found) rig_translation(L, L.sCandR[L.sOrder[0]], bestRm, bestT); // the cheapest candidate stands in
            if (lane == 0) {
                B.found = found;
                for (int k = 0; k < 9; k++) B.Rm[k] = bestRm[k];
                for (int k = 0; k < 3; k++) B.T[k] = bestT[k];
                for (int cc = 0; cc < 3; cc++)
                    for (int rr = 0; rr < 3; rr++) B.r[cc * 3 + rr] = bestRm[rr * 3 + cc];
            }
        }
        __syncthreads();
        if (final_pass || plain_only) break;
        rig_tag_rho(L, pts, n_tags, B.Rm, B.T, B.rho, lane, RIG_NT);
        __syncthreads();
        if (lane == 0) {
            double m = B.rho[0];
            for (int j = 1; j < n_tags; j++)
                if (B.rho[j] > m) m = B.rho[j];
            B.rho_max = m;
        }
        __syncthreads();
        const double rho_max = B.rho_max;
        if (rho_max <= c2) break; // the gate: every tag is an inlier, the record is this solve's
        double mu = c2 / (2.0 * rho_max - c2);
        for (;;) {
            if (lane < 64) { // the weights of this round, and whether it is one: 0 go on, 1 settled (or nothing left), 2 out of rounds
                bool binary = true, same = true, alive = false;
                for (int j = lane; j < n_tags; j += 64) {
                    const double wn = gnc_weight(B.rho[j], mu, c, c2);
                    if (wn != 0.0 && wn != 1.0) binary = false;
                    if (wn != B.wt[j]) same = false;
                    if (wn > 0.0) alive = true;
                    B.wt[j] = wn;
                }
                const bool settled = (!__ballot(!binary) && !__ballot(!same)) || !__ballot(alive);
                if (lane == 0) B.verdict = settled ? 1 : (rounds == ra.max_rounds ? 2 : 0);
            }
            __syncthreads();
            const int verdict = B.verdict;
            if (verdict) { maxed = verdict == 2; break; }
            rig_accumulate<true>(L, pts, n, B.wt, weighted, lane);
            rig_reduce(L, false, lane);
            if (lane < 16) { // one refinement from the rotation next to the last round's r
                double start[9], r[9];
                for (int k = 0; k < 9; k++) start[k] = B.r[k];
                // (both inlined here too: as calls they would take r through private memory)
                [[clang::always_inline]] nearest_so3(start, r);
                [[clang::always_inline]] (void)optimization16<true>(a.prm.sqpnp.max_iter, a.prm.sqpnp.tol_sq, r, L.sOmega, L.sG, lane);
                if (lane == 0) { // (r through LDS: rig_translation indexes it in loops, and a lane's own array would turn private)
                    for (int k = 0; k < 9; k++) B.r[k] = r[k];
                    double Rm[9], t[3];
                    rig_translation(L, B.r, Rm, t);
                    for (int k = 0; k < 9; k++) B.Rm[k] = Rm[k];
                    for (int k = 0; k < 3; k++) B.T[k] = t[k];
                }
            }
            __syncthreads();
            rig_tag_rho(L, pts, n_tags, B.Rm, B.T, B.rho, lane, RIG_NT);
            mu *= ra.mu_factor;
            rounds++;
            __syncthreads();
        }
        // the inliers: weights of 0 and 1 from here on, the masks, the counts
        for (int j = lane; j < n_tags; j += RIG_NT) B.wt[j] = (maxed ? B.wt[j] >= 0.5 : B.wt[j] == 1.0) ? 1.0 : 0.0;
        __syncthreads();
        if (lane < CK_RIG_MAX_CAMS) {
            uint64_t mask = 0;
            for (int t = 0; t < (L.sCnt[lane] >> 2); t++)
                if (B.wt[(L.sBase[lane] >> 2) + t] == 0.0) mask |= (uint64_t)1 << t;
            out->rejected[lane] = mask;
            int n_rej = 0;
            for (int cc = 0; cc < CK_RIG_MAX_CAMS; cc++) n_rej += __popcll(__shfl(mask, cc));
            if (lane == 0) {
                B.n_in = n_tags - n_rej;
                out->n_rejected = n_rej;
                out->rounds = rounds;
                out->status = B.n_in < ra.min_inlier_tags ? CK_RIG_ROBUST_NO_CONSENSUS
                              : maxed ? CK_RIG_ROBUST_MAXROUNDS : (n_rej ? CK_RIG_ROBUST_REJECTED : CK_RIG_ROBUST_CLEAN);
            }
        }
        __syncthreads();
        if (B.n_in < ra.min_inlier_tags) return; // uniform: no pose
    }
    if (lane >= 64) return;
    if (rounds == 0 && n_tags < ra.min_inlier_tags) { // (no round ran: nothing but zeroes in the record yet)
        if (lane == 0) out->status = CK_RIG_ROBUST_NO_CONSENSUS;
        return;
    }
    if (!B.found) return;
    double bestRm[9], bestT[3], bestR[9];
    for (int k = 0; k < 9; k++) bestRm[k] = B.Rm[k];
    for (int k = 0; k < 3; k++) bestT[k] = B.T[k];
    rig_finish<true>(a, L, pts, B.wt, weighted, step, lane, gyro, bestRm, bestT, bestR, &out->fused);
    if (plain_only) return;
    // sqrt(rho) of the worst tag kept and of the best one dropped, at the pose that is returned (before the pivot)
    rig_tag_rho(L, pts, n_tags, bestR, bestT, B.rho, lane, 64);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (lane != 0) return;
    double worst = 0.0, best = DBL_MAX;
    bool any = false;
    for (int j = 0; j < n_tags; j++) {
        if (B.wt[j] != 0.0) { if (B.rho[j] > worst) worst = B.rho[j]; }
        else { any = true; if (B.rho[j] < best) best = B.rho[j]; }
    }
    out->worst_inlier_rad = sqrt(worst);
    out->best_rejected_rad = any ? sqrt(best) : 0.0;
}

// k_rig, or with the robust parameters k_rig_robust (its records in d_rres), over the same arguments
static void rig_launch(ck_rig_ws *ws, const RigArgs &a, const ck_rig_robust_params_t *rp, hipStream_t stream) {
    if (!rp) { hipLaunchKernelGGL(k_rig, dim3((unsigned)a.n), dim3(RIG_NT), 0, stream, a); return; }
    RigRobustArgs ra;
    memset(&ra, 0, sizeof ra);
    ra.a = a;
    ra.a.prm = rp->rig;
    ra.gate_rad = rp->gate_rad; ra.mu_factor = rp->mu_factor; ra.max_rounds = rp->max_rounds; ra.min_inlier_tags = rp->min_inlier_tags;
    ra.out = ws->d_rres;
    hipLaunchKernelGGL(k_rig_robust, dim3((unsigned)a.n), dim3(RIG_NT), 0, stream, ra);
}

// what the kernel needs on the device besides the cameras' arrays: results, gyro, the points of the first pass
static int rig_reserve(ck_rig_ws *ws, int n, int max_points, bool robust) {
    int rc;
    if (robust && (rc = ws->d_rres.reserve(sizeof(ck_rig_robust_result_t) * (size_t)n)) != CK_OK) return rc;
    if ((rc = ws->d_points.reserve(sizeof(double) * CK_RIG_POINT_DOUBLES * (size_t)n * (size_t)(max_points > 0 ? max_points : 1))) != CK_OK) return rc;
    if ((rc = ws->d_res.reserve(sizeof(ck_rig_result_t) * (size_t)n)) != CK_OK) return rc;
    return ws->d_gyro.reserve(sizeof(double) * (size_t)n);
}

} // namespace

// ck_rig_solve_batch (rp null, out: ck_rig_result_t[n]) and ck_rig_solve_robust_batch (params = &rp->rig, out: ck_rig_robust_result_t[n])
static int rig_solve_batch(ck_handle_t *h, const ck_rig_params_t *params, const ck_rig_robust_params_t *rp, int32_t n_cams,
                           const ck_sqpnp_problem_t *problems, int32_t n, const ck_iso3_t *tags, int32_t n_tags_total, const double *bearings,
                           int32_t n_bearings_total, const double *gyro, void *out) {
    if (!h || !params || !problems || n < 0 || n_cams < 1 || n_cams > CK_RIG_MAX_CAMS) return CK_EINVAL;
    if (n == 0) {
        const int rc = ck_rig_check(params, n_cams, problems, 0, tags, n_tags_total, bearings, n_bearings_total, gyro, out, nullptr);
        return rc != CK_OK || !rp ? rc : ck_rig_robust_check(rp, n_cams, nullptr, 0);
    }
    CK_HIP(hipSetDevice(h->device));
    // the records may lie on the device: the checks read a host copy
    std::vector<ck_sqpnp_problem_t> rec((size_t)n_cams * (size_t)n);
    CK_HIP(hipMemcpy(rec.data(), problems, sizeof(ck_sqpnp_problem_t) * rec.size(), hipMemcpyDefault));
    int32_t max_points = 0;
    int rc = ck_rig_check(params, n_cams, rec.data(), n, tags, n_tags_total, bearings, n_bearings_total, gyro, out, &max_points);
    if (rc != CK_OK) return rc;
    if (rp && (rc = ck_rig_robust_check(rp, n_cams, rec.data(), n)) != CK_OK) return rc;
    ck_rig_ws *ws = ck_workspace(h->rig);
    if (!ws) return CK_ENOMEM;
    if ((rc = rig_reserve(ws, n, max_points, rp != nullptr)) != CK_OK) return rc;
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
    rig_launch(ws, a, rp, h->stream);
    CK_HIP(hipGetLastError());
    if (rp) CK_HIP(hipMemcpyAsync(out, ws->d_rres, sizeof(ck_rig_robust_result_t) * (size_t)n, hipMemcpyDefault, h->stream));
    else CK_HIP(hipMemcpyAsync(out, ws->d_res, sizeof(ck_rig_result_t) * (size_t)n, hipMemcpyDefault, h->stream));
    CK_HIP(hipStreamSynchronize(h->stream)); // (rec, a pageable source of the first copy, lives until here)
    return CK_OK;
}

extern "C" int ck_rig_solve_batch(ck_handle_t *h, const ck_rig_params_t *params, int32_t n_cams, const ck_sqpnp_problem_t *problems, int32_t n,
                                  const ck_iso3_t *tags, int32_t n_tags_total, const double *bearings, int32_t n_bearings_total,
                                  const double *gyro, ck_rig_result_t *out) {
    return rig_solve_batch(h, params, nullptr, n_cams, problems, n, tags, n_tags_total, bearings, n_bearings_total, gyro, out);
}

extern "C" int ck_rig_solve_robust_batch(ck_handle_t *h, const ck_rig_robust_params_t *params, int32_t n_cams, const ck_sqpnp_problem_t *problems,
                                         int32_t n, const ck_iso3_t *tags, int32_t n_tags_total, const double *bearings,
                                         int32_t n_bearings_total, const double *gyro, ck_rig_robust_result_t *out) {
    if (!params) return CK_EINVAL;
    return rig_solve_batch(h, &params->rig, params, n_cams, problems, n, tags, n_tags_total, bearings, n_bearings_total, gyro, out);
}

// Measurement aid (ck_rig_refine_time): k_rig once more over the arrays the last ck_rig_solve_batch of this shape left in the workspace
int ck_rig_relaunch_batch(ck_handle_t *h, const ck_rig_params_t *params, int32_t n_cams, int32_t n, int32_t max_points) {
    ck_rig_ws *ws = h->rig;
    if (!ws || n < 1) return CK_EINVAL;
    RigArgs a;
    memset(&a, 0, sizeof a);
    a.prm = *params;
    for (int c = 0; c < n_cams; c++) a.cam[c] = {ws->d_prob.p + (size_t)c * n, ws->d_tags, ws->d_bearings, nullptr, 0, 0};
    a.n_cams = n_cams; a.n = n; a.max_points = max_points;
    a.gyro = ws->d_gyro; a.points = ws->d_points; a.out = ws->d_res;
    rig_launch(ws, a, nullptr, h->stream);
    CK_HIP(hipGetLastError());
    return CK_OK;
}

// ck_rig_process_last up to, not including, the wait for the stream
// (rp: the robust solve, params = &rp->rig and out a ck_rig_robust_result_t[n]); ck_rig_process_last_refined (ck_rig_refine.hip) goes on from here
int ck_rig_enqueue_last(ck_handle_t *const *handles, int32_t n_cams, int32_t n, const ck_rig_params_t *params,
                            const ck_rig_robust_params_t *rp, const double *gyro, const uint8_t *has_gyro, void *out,
                            ck_vision_measurement_t *meas, int32_t *valid) {
    if (rp && ck_rig_robust_check(rp, 0, nullptr, 0) != CK_OK) return CK_EINVAL;
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
    int rc = rig_reserve(ws, n, max_points, rp != nullptr);
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
    rig_launch(ws, a, rp, h->stream);
    CK_HIP(hipGetLastError());
    if (out && rp) CK_HIP(hipMemcpyAsync(out, ws->d_rres, sizeof(ck_rig_robust_result_t) * (size_t)n, hipMemcpyDefault, h->stream));
    else if (out) CK_HIP(hipMemcpyAsync(out, ws->d_res, sizeof(ck_rig_result_t) * (size_t)n, hipMemcpyDefault, h->stream));
    CK_HIP(hipMemcpyAsync(meas, ws->d_meas, sizeof(ck_vision_measurement_t) * (size_t)n, hipMemcpyDefault, h->stream));
    CK_HIP(hipMemcpyAsync(valid, ws->d_valid, sizeof(int32_t) * (size_t)n, hipMemcpyDefault, h->stream));
    return CK_OK;
}

extern "C" int ck_rig_process_last(ck_handle_t *const *handles, int32_t n_cams, int32_t n, const ck_rig_params_t *params, const double *gyro,
                                   const uint8_t *has_gyro, ck_rig_result_t *out, ck_vision_measurement_t *meas, int32_t *valid) {
    const int rc = ck_rig_enqueue_last(handles, n_cams, n, params, nullptr, gyro, has_gyro, out, meas, valid);
    if (rc != CK_OK) return rc;
    CK_HIP(hipStreamSynchronize(handles[0]->stream));
    return CK_OK;
}

extern "C" int ck_rig_process_last_robust(ck_handle_t *const *handles, int32_t n_cams, int32_t n, const ck_rig_robust_params_t *params,
                                          const double *gyro, const uint8_t *has_gyro, ck_rig_robust_result_t *out,
                                          ck_vision_measurement_t *meas, int32_t *valid) {
    if (!params) return CK_EINVAL;
    const int rc = ck_rig_enqueue_last(handles, n_cams, n, &params->rig, params, gyro, has_gyro, out, meas, valid);
    if (rc != CK_OK) return rc;
    CK_HIP(hipStreamSynchronize(handles[0]->stream));
    return CK_OK;
}

extern "C" int ck_rig_time_last(ck_handle_t *const *handles, int32_t n_cams, int32_t n, const ck_rig_params_t *params, const double *gyro,
                                const uint8_t *has_gyro, int32_t iters, float *ms_rig, float *ms_sqpnp) {
    if (iters < 1 || !ms_rig || !ms_sqpnp || n < 1) return CK_EINVAL;
    std::vector<ck_vision_measurement_t> meas((size_t)n);
    std::vector<int32_t> valid((size_t)n);
    int rc = ck_rig_enqueue_last(handles, n_cams, n, params, nullptr, gyro, has_gyro, nullptr, meas.data(), valid.data()); // (checks, workspace)
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
            if (which == 0) rc = ck_rig_enqueue_last(handles, n_cams, n, params, nullptr, gyro, has_gyro, nullptr, meas.data(), valid.data());
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
