// k_fieldcal.hip — Levenberg-Marquardt refinement of the field's tag poses and one robot pose per step: one persistent
// workgroup of 256 threads per problem, the whole iteration inside the kernel.  The arithmetic is ck_fieldcal_math.h's and, shared with
// the mount calibration, ck_cal_math.h's, the same text the host twin (ck_fieldcal_host.c) compiles; this file only decides who
// computes what.
//   points          a group of 4 lanes takes the sightings group, group + 64, ... of the problem, in rounds that every group of the
//                   workgroup walks together; lane l has corner l.  The 4 values meet in the xor butterfly 2, 1, which stands OUTSIDE
//                   "has this group a sighting": every lane is active at every exchange (k_tail).  The 90 sums of a
//                   sighting are formed in two passes so that they stay in registers; lane 0 writes them into the sighting's record
//   pairs, steps    thread t takes the pairs t, t + 256, ... (adds a pair's sightings in camera order) and then the used steps
//                   t, t + 256, ...: adds the step's pairs in tag order, factors the 6 x 6 block and leaves W = L^-1 B^T in every pair's
//                   record.  No thread keeps sums per tag: an accumulator indexed by a runtime tag number would live in private memory
//   reduced system  6 T <= 384 unknowns, the packed lower triangle in the call's global workspace (1.2 MB at the cap: not LDS).
//                   Thread e, e + 256, ... sums one entry over the steps in order.  Left-looking column Cholesky by the whole
//                   workgroup: thread t owns the rows t and t + 256; for column j the row j of L is staged in LDS and every owned row
//                   i >= j subtracts its products in increasing c, alone.  The substitutions sweep the columns and each owned row
//                   subtracts one product per column: forward in increasing c, backward in decreasing c, as the twin's loops do.
//                   So every entry is the twin's, whatever the thread count.
// Plain C++ and __shfl_xor only.
#include "ck_fieldcal.h"
#include "ck_fieldcal_math.h"

namespace {

constexpr int NTH = 256, NGRP = NTH / CKF_GROUP, TMAX = CK_FIELDCAL_MAX_TAGS, NMAX = 6 * TMAX, NROW = (NMAX + NTH - 1) / NTH;

__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
    for (int m = CKF_GROUP / 2; m >= 1; m >>= 1) v = v + __shfl_xor(v, m);
    return v;
}

struct sight_t {
    bool on;
    int k;
    double M[12], P[12], T[12], b[3];
};
// the sighting g of this lane's group: its camera, step pose (at `pose_at` of the step's record), tag and this lane's bearing
__device__ __forceinline__ void sight_of(sight_t &w, int g, int NS, const ckf_meta_t &m, const double *s_M, const double *s_T,
                                         const double *__restrict__ steps, int pose_at, const double *__restrict__ bear, int lane) {
    w.on = g < NS;
    w.k = 0;
    if (w.on) {
        const int pi = m.sight_pair[g], c = m.sight_cam[g];
        w.k = m.ix.col[pi];
        const double *P = steps + (size_t)CKA_S_STRIDE * m.ix.step[pi] + pose_at;
        const double *b = bear + 3 * ((size_t)m.sight_bear[g] + lane);
#pragma unroll
        for (int i = 0; i < 12; i++) { w.M[i] = s_M[12 * c + i]; w.P[i] = P[i]; w.T[i] = s_T[12 * w.k + i]; }
#pragma unroll
        for (int i = 0; i < 3; i++) w.b[i] = b[i];
    }
}

// the candidate's squared residuals, per sighting into the records
__device__ __forceinline__ void cost_pass(const double *s_M, const double *s_Tc, const double *__restrict__ steps, double *__restrict__ sights,
                                          const ckf_meta_t &m, int NS, const double *__restrict__ bear, int group, int lane) {
    for (int g0 = 0; g0 < NS; g0 += NGRP) {
        sight_t w;
        sight_of(w, g0 + group, NS, m, s_M, s_Tc, steps, CKA_S_CAND, bear, lane);
        double a = 0.0;
        if (w.on) {
            double e[3];
            ckf_residual(w.M, w.P, w.T, lane, w.b, e);
            a = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
        }
        a = group_sum(a);
        if (lane == 0 && w.on) sights[(size_t)CKF_I_STRIDE * (g0 + group) + CKF_I_COST] = a;
    }
}

// the normal equations at the accepted parameters, per sighting into the records: the rows A0 .. A1 - 1 of the triangle, and J^T e
// with the first rows
template <int A0, int A1>
__device__ __forceinline__ void jacobian_pass(const double *s_M, const double *s_T, const int32_t *s_mask, const double *__restrict__ steps,
                                              double *__restrict__ sights, const ckf_meta_t &m, int NS, const double *__restrict__ bear,
                                              int group, int lane) {
    constexpr int NT = CKA_TRI(A1, A1) - CKA_TRI(A0, A0), NG = A0 == 0 ? CKA_NJ : 0;
    for (int g0 = 0; g0 < NS; g0 += NGRP) {
        sight_t w;
        sight_of(w, g0 + group, NS, m, s_M, s_T, steps, CKA_S_POSE, bear, lane);
        double acc[NT], g[NG ? NG : 1];
#pragma unroll
        for (int j = 0; j < NT; j++) acc[j] = 0.0;
#pragma unroll
        for (int j = 0; j < NG; j++) g[j] = 0.0;
        if (w.on) {
            double e[3], J[3 * CKA_NJ];
            ckf_jacobian(w.M, w.P, w.T, lane, w.b, (unsigned)s_mask[w.k], e, J);
            ckr_accumulate_rows(acc, NG ? g : nullptr, e, J, A0, A1);
        }
#pragma unroll
        for (int j = 0; j < NT; j++) acc[j] = group_sum(acc[j]);
#pragma unroll
        for (int j = 0; j < NG; j++) g[j] = group_sum(g[j]);
        if (lane == 0 && w.on) {
            double *V = sights + (size_t)CKF_I_STRIDE * (g0 + group);
#pragma unroll
            for (int j = 0; j < NT; j++) V[CKF_I_H + CKA_TRI(A0, A0) + j] = acc[j];
#pragma unroll
            for (int j = 0; j < NG; j++) V[CKF_I_G + j] = g[j];
        }
    }
}

// per used step the candidate's cost: its pairs in tag order, each its sightings in camera order
__device__ __forceinline__ void step_costs(double *__restrict__ steps, double *__restrict__ pairs, const double *__restrict__ sights,
                                           const ckf_meta_t &m, int U, int tid) {
    for (int u = tid; u < U; u += NTH) {
        const int p0 = m.ix.first[u];
        ckf_step_cost(steps + (size_t)CKA_S_STRIDE * u, pairs + (size_t)CKA_B_STRIDE * p0, sights + (size_t)CKF_I_STRIDE * m.pair_sight[p0],
                      m.pair_sight + p0, m.ix.first[u + 1] - p0);
    }
}

// S (packed lower triangle, global) d = rhs in place in s_dk (LDS): the factorisation and the two substitutions described above.
// Every thread of the workgroup calls it; false (for all of them) at the first pivot that is not positive.
__device__ __forceinline__ bool reduced_solve(double *S, int N, double *s_dk, double *s_col, double *s_piv, int tid) {
    for (int j = 0; j < N; j++) {
        for (int c = tid; c < j; c += NTH) s_col[c] = S[CKF_LT(j, c)];
        __syncthreads();
        double w[NROW];
#pragma unroll
        for (int h = 0; h < NROW; h++) {
            const int i = tid + h * NTH;
            w[h] = 0.0;
            if (i >= j && i < N) {
                const double *Si = S + CKF_LT(i, 0);
                double t = Si[j];
                for (int c = 0; c < j; c++) t = t - Si[c] * s_col[c];
                w[h] = t;
                if (i == j) *s_piv = t;
            }
        }
        __syncthreads();
        const double t = *s_piv;
        if (!(t > 0.0)) return false;
        const double d = sqrt(t);
#pragma unroll
        for (int h = 0; h < NROW; h++) {
            const int i = tid + h * NTH;
            if (i == j) S[CKF_LT(j, j)] = d;
            else if (i > j && i < N) S[CKF_LT(i, j)] = w[h] / d;
        }
        __syncthreads(); // row j + 1 is staged next, and the pivot's slot is written again
    }
    double t[NROW];
#pragma unroll
    for (int h = 0; h < NROW; h++) t[h] = tid + h * NTH < N ? s_dk[tid + h * NTH] : 0.0;
    __syncthreads();
    for (int c = 0; c < N; c++) {
#pragma unroll
        for (int h = 0; h < NROW; h++)
            if (tid + h * NTH == c) s_dk[c] = t[h] / S[CKF_LT(c, c)];
        __syncthreads();
        const double y = s_dk[c];
#pragma unroll
        for (int h = 0; h < NROW; h++) {
            const int i = tid + h * NTH;
            if (i > c && i < N) t[h] = t[h] - S[CKF_LT(i, c)] * y;
        }
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < NROW; h++) t[h] = tid + h * NTH < N ? s_dk[tid + h * NTH] : 0.0;
    __syncthreads();
    for (int c = N - 1; c >= 0; c--) {
#pragma unroll
        for (int h = 0; h < NROW; h++)
            if (tid + h * NTH == c) s_dk[c] = t[h] / S[CKF_LT(c, c)];
        __syncthreads();
        const double x = s_dk[c];
#pragma unroll
        for (int h = 0; h < NROW; h++) {
            const int i = tid + h * NTH;
            if (i < c) t[h] = t[h] - S[CKF_LT(c, i)] * x;
        }
    }
    __syncthreads();
    return true;
}

__global__ __launch_bounds__(NTH) void k_fieldcal(const ck_fieldcal_dev_problem *__restrict__ prob, const int32_t *__restrict__ meta_all,
                                                  const double *__restrict__ bear, const double *__restrict__ mounts,
                                                  double *__restrict__ tags_all, double *__restrict__ rms_all, double *__restrict__ steps_all,
                                                  double *__restrict__ pairs_all, double *__restrict__ sights_all, double *__restrict__ S_all,
                                                  ck_fieldcal_result_t *__restrict__ res, int C, int max_iters) {
    __shared__ double s_M[12 * CK_RIG_MAX_CAMS], s_T[12 * TMAX], s_Tc[12 * TMAX], s_Hk[CKA_HK * TMAX], s_dk[NMAX], s_col[NMAX];
    __shared__ int32_t s_mask[TMAX];
    __shared__ double s_cost0, s_piv;
    __shared__ ckc_lm_t s_lm;
    __shared__ int s_solved, s_accept;
    const int tid = threadIdx.x, lane = tid & (CKF_GROUP - 1), group = tid / CKF_GROUP;
    ck_fieldcal_result_t *R = res + blockIdx.x;
    if (R->status == CK_CALIB_DEGENERATE) return; // no start: the record stays as the host wrote it
    const ck_fieldcal_dev_problem q = prob[blockIdx.x];
    const int U = q.U, P = q.P, NS = q.NS, T = q.T, N = 6 * T, NE = (N * (N + 1)) / 2;
    const ckf_meta_t m = ckf_meta_at(meta_all + q.meta_off, (size_t)U, (size_t)P, (size_t)NS, (size_t)T);
    double *steps = steps_all + (size_t)CKA_S_STRIDE * (size_t)q.step_off;
    double *pairs = pairs_all + (size_t)CKA_B_STRIDE * (size_t)q.pair_off;
    double *sights = sights_all + (size_t)CKF_I_STRIDE * (size_t)q.sight_off;
    double *S = S_all + q.s_off;
    double *Tg = tags_all + (size_t)12 * TMAX * blockIdx.x;

    if (tid < 12 * C) s_M[tid] = mounts[tid];
    for (int i = tid; i < 12 * T; i += NTH) s_T[i] = s_Tc[i] = Tg[i];
    if (tid < T) s_mask[tid] = m.mask6[tid];
    __syncthreads();
    cost_pass(s_M, s_Tc, steps, sights, m, NS, bear, group, lane);
    __syncthreads();
    step_costs(steps, pairs, sights, m, U, tid);
    __syncthreads();
    for (int pi = tid; pi < P; pi += NTH) pairs[(size_t)CKA_B_STRIDE * pi + CKA_B_COSTA] = pairs[(size_t)CKA_B_STRIDE * pi + CKA_B_COST];
    if (tid == 0) {
        double c = 0.0;
        for (int u = 0; u < U; u++) c = c + steps[(size_t)CKA_S_STRIDE * u + CKA_S_COST];
        s_cost0 = c;
        ckc_lm_start(&s_lm, c, CKR_COST_FLOOR);
        if (!ckc_finite(c)) s_lm.status = CK_CALIB_DEGENERATE;
    }
    __syncthreads();
    if (s_lm.status == CK_CALIB_DEGENERATE) {
        if (tid == 0) R->status = CK_CALIB_DEGENERATE;
        return;
    }
    while (s_lm.status < 0) {
        const double lambda = s_lm.lambda;
        if (s_lm.need_jac) {
            jacobian_pass<0, 4>(s_M, s_T, s_mask, steps, sights, m, NS, bear, group, lane);
            jacobian_pass<4, CKA_NJ>(s_M, s_T, s_mask, steps, sights, m, NS, bear, group, lane);
            __syncthreads();
            for (int pi = tid; pi < P; pi += NTH)
                ckf_pair_sum(pairs + (size_t)CKA_B_STRIDE * pi, sights + (size_t)CKF_I_STRIDE * m.pair_sight[pi], m.pair_sight[pi + 1] - m.pair_sight[pi]);
            __syncthreads();
            for (int j = tid; j < CKA_HK * T; j += NTH) s_Hk[j] = cka_col_sum(pairs, m.ix.colmap + (size_t)(j / CKA_HK) * U, U, j % CKA_HK);
        }
        if (tid == 0) s_solved = 1;
        __syncthreads();
        for (int u = tid; u < U; u += NTH)
            if (!cka_step_schur(steps + (size_t)CKA_S_STRIDE * u, pairs + (size_t)CKA_B_STRIDE * m.ix.first[u], m.ix.first[u + 1] - m.ix.first[u], lambda))
                s_solved = 0;
        __syncthreads();
        for (int e = tid; e < NE; e += NTH) {
            const int r = cka_lt_row(e);
            S[e] = cka_reduced_entry(pairs, m.ix.colmap, s_mask, s_Hk, U, nullptr, U, lambda, r, e - (r * (r + 1)) / 2);
        }
        for (int r = tid; r < N; r += NTH) s_dk[r] = cka_reduced_rhs(pairs, m.ix.colmap, s_mask, s_Hk, U, r);
        __syncthreads();
        const bool factored = reduced_solve(S, N, s_dk, s_col, &s_piv, tid);
        double pred = 0.0, cost_new = 0.0;
        if (tid == 0) {
            if (!factored) s_solved = 0;
            else pred = cka_reduced_pred(s_mask, s_Hk, N, lambda, s_dk);
        }
        __syncthreads();
        if (s_solved) {
            if (tid < T) ckc_rigid_step(s_T + 12 * tid, s_dk + 6 * tid, (unsigned)s_mask[tid], s_Tc + 12 * tid);
            for (int u = tid; u < U; u += NTH)
                cka_step_step(steps + (size_t)CKA_S_STRIDE * u, pairs + (size_t)CKA_B_STRIDE * m.ix.first[u], m.ix.col + m.ix.first[u],
                              m.ix.first[u + 1] - m.ix.first[u], s_dk, lambda);
            __syncthreads();
            cost_pass(s_M, s_Tc, steps, sights, m, NS, bear, group, lane);
            __syncthreads();
            step_costs(steps, pairs, sights, m, U, tid);
            __syncthreads();
            if (tid == 0) {
                for (int u = 0; u < U; u++) pred = pred + steps[(size_t)CKA_S_STRIDE * u + CKA_S_PRED];
                for (int u = 0; u < U; u++) cost_new = cost_new + steps[(size_t)CKA_S_STRIDE * u + CKA_S_COST];
            }
        }
        if (tid == 0) s_accept = ckc_lm_decide(&s_lm, s_solved, pred, cost_new, max_iters, CKR_COST_FLOOR);
        __syncthreads();
        if (s_accept) {
            for (int i = tid; i < 12 * T; i += NTH) s_T[i] = s_Tc[i];
            for (int i = tid; i < 12 * U; i += NTH)
                steps[(size_t)CKA_S_STRIDE * (i / 12) + CKA_S_POSE + i % 12] = steps[(size_t)CKA_S_STRIDE * (i / 12) + CKA_S_CAND + i % 12];
            for (int pi = tid; pi < P; pi += NTH) pairs[(size_t)CKA_B_STRIDE * pi + CKA_B_COSTA] = pairs[(size_t)CKA_B_STRIDE * pi + CKA_B_COST];
        }
        __syncthreads();
    }
    for (int i = tid; i < 12 * T; i += NTH) Tg[i] = s_T[i];
    if (tid < T) rms_all[(size_t)TMAX * blockIdx.x + tid] = cka_col_rms(pairs, m.ix.colmap + (size_t)tid * U, U, 4 * m.tag_ns[tid]);
    if (tid == 0) {
        R->status = s_lm.status; R->iters = s_lm.iters;
        R->cost0 = s_cost0; R->cost = s_lm.cost;
        R->rms = sqrt(s_lm.cost / (double)R->n_points);
    }
}

} // namespace

int ck_launch_fieldcal(hipStream_t stream, int max_iters, int n_cams, const ck_fieldcal_dev_problem *d_prob, int n_problems, const int32_t *d_meta,
                       const double *d_bear, const double *d_mounts, double *d_tags, double *d_rms, double *d_steps, double *d_pairs,
                       double *d_sights, double *d_S, ck_fieldcal_result_t *d_res) {
    if (n_problems < 1) return CK_OK;
    hipLaunchKernelGGL(k_fieldcal, dim3(n_problems), dim3(NTH), 0, stream, d_prob, d_meta, d_bear, d_mounts, d_tags, d_rms, d_steps, d_pairs,
                       d_sights, d_S, d_res, n_cams, max_iters);
    CK_HIP(hipGetLastError());
    return CK_OK;
}
