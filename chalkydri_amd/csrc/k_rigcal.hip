// k_rigcal.hip — Levenberg-Marquardt refinement of the camera mounts of a rig and one robot pose per step: one
// persistent workgroup of 256 threads per problem, the whole iteration inside the kernel.  The arithmetic is ck_rigcal_math.h's and,
// shared with the field calibration, ck_cal_math.h's, the same text the host twin (ck_rigcal_host.c) compiles; this file only decides
// who computes what.  A capture is many steps of few points, so the unit of work is the VIEW, one (used step, camera) pair that has
// points, 4 .. 68 of them; the problem's arrowhead index (cka_index_t) lists the views step by step in camera order:
//   points         a group of 16 lanes takes the views group, group + 16, ... of the problem, in rounds that every group of the
//                  workgroup walks together; lane l the points l, l + 16, ... of the view; the 16 partial sums meet in the xor
//                  butterfly 8 .. 1, which stands OUTSIDE the lanes' loops and outside "has this group a view": every lane is active at
//                  every exchange (k_tail).  The 90 sums of a view are formed in two passes so that they stay in registers
//   view records   lane 0 of the group writes the view's sums into its record (global memory); no thread keeps sums per camera: an
//                  accumulator indexed by a runtime camera number would live in private memory
//   6 x 6 solves   thread t takes the used steps t, t + 256, ...: adds the step's views in camera order, factors, and leaves W = L^-1 B^T
//                  in every view's record, all in registers
//   reduced system thread j one entry of the cameras' sums, then one entry of the at most 48 x 48 reduced system (cka_reduced_entry: its
//                  sum over the steps in order) straight into LDS; thread 0 factors and solves it there (ckc_chol_n, ckc_fwd_n, ckc_bwd_n)
// Plain C++ and __shfl_xor only.
#include "ck_rigcal.h"
#include "ck_rigcal_math.h"

namespace {

constexpr int NTH = 256, NGRP = NTH / CKR_GROUP, NMAX = 6 * CK_RIG_MAX_CAMS;

__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
    for (int m = CKR_GROUP / 2; m >= 1; m >>= 1) v = v + __shfl_xor(v, m);
    return v;
}

struct view_t {
    int np, xo, bo, u, c;
};
// the view of this thread's group in the round that starts at view v0; np = 0: none
__device__ __forceinline__ view_t view_of(int v0, int group, int NV, const cka_index_t &x, const int32_t *__restrict__ tab, int n) {
    view_t w = {0, 0, 0, 0, 0};
    const int v = v0 + group;
    if (v < NV) {
        w.u = x.step[v];
        w.c = x.col[v];
        const int32_t *tb = tab + ((size_t)w.c * n + x.used[w.u]) * CKR_TAB;
        w.xo = tb[0]; w.bo = tb[1]; w.np = tb[2];
    }
    return w;
}

// the candidate's squared residuals, per view into the records
__device__ __forceinline__ void cost_pass(const double *s_Mc, const double *__restrict__ steps, double *__restrict__ views, int NV,
                                          const cka_index_t &x, const int32_t *__restrict__ tab, int n, const double *__restrict__ world,
                                          const double *__restrict__ bear, int group, int lane) {
    for (int v0 = 0; v0 < NV; v0 += NGRP) {
        const view_t w = view_of(v0, group, NV, x, tab, n);
        double a = 0.0;
        if (w.np > 0) {
            double M[12], P[12];
#pragma unroll
            for (int i = 0; i < 12; i++) M[i] = s_Mc[12 * w.c + i];
#pragma unroll
            for (int i = 0; i < 12; i++) P[i] = steps[(size_t)CKA_S_STRIDE * w.u + CKA_S_CAND + i];
            for (int i = lane; i < w.np; i += CKR_GROUP) {
                double X[3], b[3], e[3];
#pragma unroll
                for (int k = 0; k < 3; k++) { X[k] = world[3 * ((size_t)w.xo + i) + k]; b[k] = bear[3 * ((size_t)w.bo + i) + k]; }
                ckr_residual(M, P, X, b, e);
                a = a + ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
            }
        }
        a = group_sum(a);
        if (lane == 0 && w.np > 0) views[(size_t)CKA_B_STRIDE * (v0 + group) + CKA_B_COST] = a;
    }
}

// the normal equations at the accepted parameters, per view into the records: the rows A0 .. A1 - 1 of the triangle, and J^T e with
// the first rows
template <int A0, int A1>
__device__ __forceinline__ void jacobian_pass(const double *s_M, const int32_t *s_mask, const double *__restrict__ steps, double *__restrict__ views,
                                              int NV, const cka_index_t &x, const int32_t *__restrict__ tab, int n,
                                              const double *__restrict__ world, const double *__restrict__ bear, int group, int lane) {
    constexpr int NT = CKA_TRI(A1, A1) - CKA_TRI(A0, A0), NG = A0 == 0 ? CKA_NJ : 0;
    for (int v0 = 0; v0 < NV; v0 += NGRP) {
        const view_t w = view_of(v0, group, NV, x, tab, n);
        double acc[NT], g[NG ? NG : 1];
#pragma unroll
        for (int j = 0; j < NT; j++) acc[j] = 0.0;
#pragma unroll
        for (int j = 0; j < NG; j++) g[j] = 0.0;
        if (w.np > 0) {
            double M[12], P[12];
#pragma unroll
            for (int i = 0; i < 12; i++) M[i] = s_M[12 * w.c + i];
#pragma unroll
            for (int i = 0; i < 12; i++) P[i] = steps[(size_t)CKA_S_STRIDE * w.u + CKA_S_POSE + i];
            const unsigned mask6 = (unsigned)s_mask[w.c];
            for (int i = lane; i < w.np; i += CKR_GROUP) {
                double X[3], b[3], e[3], J[3 * CKA_NJ];
#pragma unroll
                for (int k = 0; k < 3; k++) { X[k] = world[3 * ((size_t)w.xo + i) + k]; b[k] = bear[3 * ((size_t)w.bo + i) + k]; }
                ckr_jacobian(M, P, X, b, mask6, e, J);
                ckr_accumulate_rows(acc, NG ? g : nullptr, e, J, A0, A1);
            }
        }
#pragma unroll
        for (int j = 0; j < NT; j++) acc[j] = group_sum(acc[j]);
#pragma unroll
        for (int j = 0; j < NG; j++) g[j] = group_sum(g[j]);
        if (lane == 0 && w.np > 0) {
            double *V = views + (size_t)CKA_B_STRIDE * (v0 + group);
#pragma unroll
            for (int j = 0; j < NT; j++) V[CKA_B_H + CKA_TRI(A0, A0) + j] = acc[j];
#pragma unroll
            for (int j = 0; j < NG; j++) V[CKA_B_G + j] = g[j];
        }
    }
}

// per used step the candidate's cost: its views in camera order
__device__ __forceinline__ void step_costs(double *__restrict__ steps, const double *__restrict__ views, int U, const cka_index_t &x, int tid) {
    for (int u = tid; u < U; u += NTH) {
        double t = 0.0;
        for (int v = x.first[u]; v < x.first[u + 1]; v++) t = t + views[(size_t)CKA_B_STRIDE * v + CKA_B_COST];
        steps[(size_t)CKA_S_STRIDE * u + CKA_S_COST] = t;
    }
}

__global__ __launch_bounds__(NTH) void k_rigcal(const ck_rigcal_dev_problem *__restrict__ prob, const int32_t *__restrict__ tab,
                                                const int32_t *__restrict__ index_all, const double *__restrict__ world,
                                                const double *__restrict__ bear, double *__restrict__ mounts, double *__restrict__ steps_all,
                                                double *__restrict__ views_all, ck_rigcal_result_t *__restrict__ res, int C, int n, int max_iters) {
    __shared__ double s_M[12 * CK_RIG_MAX_CAMS], s_Mc[12 * CK_RIG_MAX_CAMS], s_dk[NMAX], s_Hc[CKA_HK * CK_RIG_MAX_CAMS], s_S[NMAX * NMAX];
    __shared__ int32_t s_mask[CK_RIG_MAX_CAMS];
    __shared__ double s_cost0;
    __shared__ ckc_lm_t s_lm;
    __shared__ int s_solved, s_accept;
    const int tid = threadIdx.x, lane = tid & (CKR_GROUP - 1), group = tid / CKR_GROUP;
    ck_rigcal_result_t *R = res + blockIdx.x;
    if (R->status == CK_CALIB_DEGENERATE) return; // no start: the record stays as the host wrote it
    const ck_rigcal_dev_problem q = prob[blockIdx.x];
    const int U = q.n_used, NV = q.n_views, N = 6 * C, NE = (N * (N + 1)) / 2;
    const cka_index_t x = cka_index_at(index_all + q.index_off, (size_t)U, (size_t)NV);
    double *steps = steps_all + (size_t)CKA_S_STRIDE * (size_t)q.step_off;
    double *views = views_all + (size_t)CKA_B_STRIDE * (size_t)q.view_off;
    double *Mg = mounts + (size_t)12 * CK_RIG_MAX_CAMS * blockIdx.x;

    if (tid < 12 * C) s_M[tid] = s_Mc[tid] = Mg[tid];
    if (tid < C) s_mask[tid] = (int32_t)((q.mask >> (6 * tid)) & 63u);
    __syncthreads();
    cost_pass(s_Mc, steps, views, NV, x, tab, n, world, bear, group, lane);
    __syncthreads();
    step_costs(steps, views, U, x, tid);
    for (int v = tid; v < NV; v += NTH) views[(size_t)CKA_B_STRIDE * v + CKA_B_COSTA] = views[(size_t)CKA_B_STRIDE * v + CKA_B_COST];
    __syncthreads();
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
            jacobian_pass<0, 4>(s_M, s_mask, steps, views, NV, x, tab, n, world, bear, group, lane);
            jacobian_pass<4, CKA_NJ>(s_M, s_mask, steps, views, NV, x, tab, n, world, bear, group, lane);
            __syncthreads();
            if (tid < CKA_HK * C) s_Hc[tid] = cka_col_sum(views, x.colmap + (size_t)(tid / CKA_HK) * U, U, tid % CKA_HK);
        }
        if (tid == 0) s_solved = 1;
        __syncthreads();
        for (int u = tid; u < U; u += NTH)
            if (!cka_step_schur(steps + (size_t)CKA_S_STRIDE * u, views + (size_t)CKA_B_STRIDE * x.first[u], x.first[u + 1] - x.first[u], lambda)) s_solved = 0;
        __syncthreads();
        for (int e = tid; e < NE; e += NTH) {
            const int r = cka_lt_row(e), k = e - (r * (r + 1)) / 2;
            s_S[r * N + k] = cka_reduced_entry(views, x.colmap, s_mask, s_Hc, U, nullptr, U, lambda, r, k);
        }
        if (tid < N) s_dk[tid] = cka_reduced_rhs(views, x.colmap, s_mask, s_Hc, U, tid);
        __syncthreads();
        double pred = 0.0, cost_new = 0.0;
        if (tid == 0) { // at most 48 unknowns: one thread, ck_cal_math.h says why this solve is not §4m's
            if (!ckc_chol_n(s_S, N)) s_solved = 0;
            ckc_fwd_n(s_S, N, s_dk, 1);
            ckc_bwd_n(s_S, N, s_dk);
            pred = cka_reduced_pred(s_mask, s_Hc, N, lambda, s_dk);
        }
        __syncthreads();
        if (s_solved) {
            if (tid < C) ckc_rigid_step(s_M + 12 * tid, s_dk + 6 * tid, (unsigned)s_mask[tid], s_Mc + 12 * tid);
            for (int u = tid; u < U; u += NTH)
                cka_step_step(steps + (size_t)CKA_S_STRIDE * u, views + (size_t)CKA_B_STRIDE * x.first[u], x.col + x.first[u], x.first[u + 1] - x.first[u],
                              s_dk, lambda);
            __syncthreads();
            cost_pass(s_Mc, steps, views, NV, x, tab, n, world, bear, group, lane);
            __syncthreads();
            step_costs(steps, views, U, x, tid);
            __syncthreads();
            if (tid == 0) {
                for (int u = 0; u < U; u++) pred = pred + steps[(size_t)CKA_S_STRIDE * u + CKA_S_PRED];
                for (int u = 0; u < U; u++) cost_new = cost_new + steps[(size_t)CKA_S_STRIDE * u + CKA_S_COST];
            }
        }
        if (tid == 0) s_accept = ckc_lm_decide(&s_lm, s_solved, pred, cost_new, max_iters, CKR_COST_FLOOR);
        __syncthreads();
        if (s_accept) {
            if (tid < 12 * C) s_M[tid] = s_Mc[tid];
            for (int i = tid; i < 12 * U; i += NTH)
                steps[(size_t)CKA_S_STRIDE * (i / 12) + CKA_S_POSE + i % 12] = steps[(size_t)CKA_S_STRIDE * (i / 12) + CKA_S_CAND + i % 12];
            for (int v = tid; v < NV; v += NTH) views[(size_t)CKA_B_STRIDE * v + CKA_B_COSTA] = views[(size_t)CKA_B_STRIDE * v + CKA_B_COST];
        }
        __syncthreads();
    }
    if (tid < 12 * C) Mg[tid] = s_M[tid];
    if (tid < C && R->cam_points[tid] > 0) R->cam_rms[tid] = cka_col_rms(views, x.colmap + (size_t)tid * U, U, R->cam_points[tid]);
    if (tid == 0) {
        R->status = s_lm.status; R->iters = s_lm.iters;
        R->cost0 = s_cost0; R->cost = s_lm.cost;
        R->rms = sqrt(s_lm.cost / (double)R->n_points);
    }
}

} // namespace

int ck_launch_rigcal(hipStream_t stream, int max_iters, int n_cams, int n_steps, const ck_rigcal_dev_problem *d_prob, int n_problems,
                     const int32_t *d_tab, const int32_t *d_index, const double *d_world, const double *d_bear, double *d_mounts,
                     double *d_steps, double *d_views, ck_rigcal_result_t *d_res) {
    if (n_problems < 1) return CK_OK;
    hipLaunchKernelGGL(k_rigcal, dim3(n_problems), dim3(NTH), 0, stream, d_prob, d_tab, d_index, d_world, d_bear, d_mounts, d_steps, d_views,
                       d_res, n_cams, n_steps, max_iters);
    CK_HIP(hipGetLastError());
    return CK_OK;
}
