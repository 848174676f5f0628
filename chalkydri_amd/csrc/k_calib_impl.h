// k_calib_impl.h — the calibration kernel as a template over the camera model, included by the two translation
// units that instantiate it: k_calib.hip (OpenCVModel5) and k_calib_eucm.hip (EUCM / UCM).  One kernel per translation unit: with both
// in one, the compiler's choices for the OpenCVModel5 kernel move (two more registers, four spills, 600 bytes more LDS), and that
// kernel's code is to stay what it was.
#ifndef K_CALIB_IMPL_H
#define K_CALIB_IMPL_H

#include "ck_calib.h"
#include "ck_calib_math.h"

namespace {

constexpr int NTH = 256, NW = NTH / 64;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m);
    return v;
}

// the candidate's squared residuals, per frame into the records
template <int MODEL>
__device__ __forceinline__ void cost_pass(const double *__restrict__ s_kc, double *__restrict__ rec, int F, const int32_t *__restrict__ fs,
                                          const double *__restrict__ bxy, const double *__restrict__ uv, int wave, int lane) {
    double k[9];
#pragma unroll
    for (int i = 0; i < 9; i++) k[i] = s_kc[i];
    for (int f = wave; f < F; f += NW) {
        double *wf = rec + (size_t)CKC_WS_STRIDE * f;
        double P[12];
#pragma unroll
        for (int i = 0; i < 12; i++) P[i] = wf[CKC_WS_CAND + i];
        double c = 0.0;
        const int end = fs[f + 1];
        for (int i = fs[f] + lane; i < end; i += 64) {
            double r[2];
            ckc_residual_of(MODEL, k, P, bxy[2 * i], bxy[2 * i + 1], uv[2 * i], uv[2 * i + 1], r);
            c = c + (r[0] * r[0] + r[1] * r[1]);
        }
        c = wave_sum(c);
        if (lane == 0) wf[CKC_WS_COST] = c;
    }
}

// the normal equations at the accepted parameters, per frame into the records: the rows A0 .. A1 - 1 of the triangle, and J^T r with
// the first rows
template <int MODEL, int A0, int A1>
__device__ __forceinline__ void jacobian_pass(const double *__restrict__ s_k, double *__restrict__ rec, int F, const int32_t *__restrict__ fs,
                                              const double *__restrict__ bxy, const double *__restrict__ uv, unsigned fixed_mask, int wave,
                                              int lane) {
    double k[9];
#pragma unroll
    for (int i = 0; i < 9; i++) k[i] = s_k[i];
    for (int f = wave; f < F; f += NW) {
        double *wf = rec + (size_t)CKC_WS_STRIDE * f;
        constexpr int NT = CKC_TRI(A1, A1) - CKC_TRI(A0, A0), NG = A0 == 0 ? CKC_NJ : 0;
        double P[12], acc[NT], g[NG ? NG : 1];
#pragma unroll
        for (int i = 0; i < 12; i++) P[i] = wf[CKC_WS_POSE + i];
#pragma unroll
        for (int j = 0; j < NT; j++) acc[j] = 0.0;
#pragma unroll
        for (int j = 0; j < NG; j++) g[j] = 0.0;
        const int end = fs[f + 1];
        for (int i = fs[f] + lane; i < end; i += 64) {
            double r[2], Ju[CKC_NJ], Jv[CKC_NJ];
            ckc_jacobian_of(MODEL, k, P, bxy[2 * i], bxy[2 * i + 1], uv[2 * i], uv[2 * i + 1], fixed_mask, r, Ju, Jv);
            ckc_accumulate_rows(acc, NG ? g : nullptr, r, Ju, Jv, A0, A1);
        }
#pragma unroll
        for (int j = 0; j < NT; j++) acc[j] = wave_sum(acc[j]);
#pragma unroll
        for (int j = 0; j < NG; j++) g[j] = wave_sum(g[j]);
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < NT; j++) wf[CKC_WS_H + CKC_TRI(A0, A0) + j] = acc[j];
#pragma unroll
            for (int j = 0; j < NG; j++) wf[CKC_WS_H + CKC_NH + j] = g[j];
        }
    }
}

// out[j] = entry off + j of the records, added in frame order
__device__ __forceinline__ void frame_sum(double *out, int n, const double *rec, int off, int F, int tid) {
    if (tid < n) {
        double s = 0.0;
        for (int f = 0; f < F; f++) s = s + rec[(size_t)CKC_WS_STRIDE * f + off + tid];
        out[tid] = s;
    }
}

template <int MODEL>
__global__ __launch_bounds__(NTH) void k_calib(const ck_calib_problem_t *__restrict__ prob, const int32_t *__restrict__ rec0,
                                               const int32_t *__restrict__ frame_start, const double *__restrict__ board_xy,
                                               const double *__restrict__ image_uv, double *__restrict__ recs, double *__restrict__ poses,
                                               ck_calib_result_t *__restrict__ res, unsigned fixed_mask, int max_iters) {
    __shared__ double s_k[9], s_kc[9], s_dk[9], s_Hs[CKC_NACC], s_Es[54], s_S[81];
    __shared__ double s_cost0;
    __shared__ ckc_lm_t s_lm;
    __shared__ int s_solved, s_accept;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    ck_calib_result_t *R = res + blockIdx.x;
    if (R->status == CK_CALIB_DEGENERATE) return; // no start: the record stays as the host wrote it
    const ck_calib_problem_t q = prob[blockIdx.x];
    const int F = q.n_frames;
    const int32_t *fs = frame_start + q.start_offset;
    const double *bxy = board_xy + 2 * (size_t)q.point_offset, *uv = image_uv + 2 * (size_t)q.point_offset;
    double *rec = recs + (size_t)CKC_WS_STRIDE * (size_t)rec0[blockIdx.x];
    double *P = poses + 12 * (size_t)q.pose_offset;

    if (tid < 9) s_k[tid] = s_kc[tid] = ((const double *)&R->cam)[tid];
    for (int i = tid; i < 12 * F; i += NTH) {
        const double v = P[i];
        rec[(size_t)CKC_WS_STRIDE * (i / 12) + CKC_WS_POSE + i % 12] = v;
        rec[(size_t)CKC_WS_STRIDE * (i / 12) + CKC_WS_CAND + i % 12] = v;
    }
    __syncthreads();
    cost_pass<MODEL>(s_kc, rec, F, fs, bxy, uv, wave, lane);
    __syncthreads();
    if (tid == 0) {
        double c = 0.0;
        for (int f = 0; f < F; f++) c = c + rec[(size_t)CKC_WS_STRIDE * f + CKC_WS_COST];
        s_cost0 = c;
        ckc_lm_start(&s_lm, c, CKC_COST_FLOOR);
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
            jacobian_pass<MODEL, 0, 5>(s_k, rec, F, fs, bxy, uv, fixed_mask, wave, lane);
            jacobian_pass<MODEL, 5, CKC_NJ>(s_k, rec, F, fs, bxy, uv, fixed_mask, wave, lane);
            __syncthreads();
            frame_sum(s_Hs, CKC_NACC, rec, CKC_WS_H, F, tid);
        }
        if (tid == 0) s_solved = 1;
        __syncthreads();
        for (int f = tid; f < F; f += NTH)
            if (!ckc_frame_schur(rec + (size_t)CKC_WS_STRIDE * f, lambda)) s_solved = 0;
        __syncthreads();
        frame_sum(s_Es, 54, rec, CKC_WS_E, F, tid);
        __syncthreads();
        double pred = 0.0, cost_new = 0.0;
        if (tid == 0) {
            if (!ckc_reduced_solve(s_Hs, s_Es, lambda, fixed_mask, s_S, s_dk, &pred)) s_solved = 0;
            for (int i = 0; i < 9; i++) s_kc[i] = ((fixed_mask >> i) & 1u) ? s_k[i] : s_k[i] + s_dk[i];
        }
        __syncthreads();
        if (s_solved) {
            for (int f = tid; f < F; f += NTH) ckc_frame_step(rec + (size_t)CKC_WS_STRIDE * f, s_dk, lambda);
            __syncthreads();
            cost_pass<MODEL>(s_kc, rec, F, fs, bxy, uv, wave, lane);
            __syncthreads();
            if (tid == 0) {
                for (int f = 0; f < F; f++) pred = pred + rec[(size_t)CKC_WS_STRIDE * f + CKC_WS_PRED];
                for (int f = 0; f < F; f++) cost_new = cost_new + rec[(size_t)CKC_WS_STRIDE * f + CKC_WS_COST];
            }
        }
        if (tid == 0) {
            s_accept = ckc_lm_decide(&s_lm, s_solved, pred, cost_new, max_iters, CKC_COST_FLOOR);
            if (s_accept)
                for (int i = 0; i < 9; i++) s_k[i] = s_kc[i];
        }
        __syncthreads();
        if (s_accept)
            for (int i = tid; i < 12 * F; i += NTH)
                rec[(size_t)CKC_WS_STRIDE * (i / 12) + CKC_WS_POSE + i % 12] = rec[(size_t)CKC_WS_STRIDE * (i / 12) + CKC_WS_CAND + i % 12];
        __syncthreads();
    }
    for (int i = tid; i < 12 * F; i += NTH) P[i] = rec[(size_t)CKC_WS_STRIDE * (i / 12) + CKC_WS_POSE + i % 12];
    if (tid < 9) ((double *)&R->cam)[tid] = s_k[tid];
    if (tid == 0) {
        R->status = s_lm.status; R->iters = s_lm.iters;
        R->cost0 = s_cost0; R->cost = s_lm.cost;
        R->rms = sqrt(s_lm.cost / (double)R->n_points);
    }
}

} // namespace

template <int MODEL>
static int launch_calib_model(hipStream_t stream, const ck_calib_params_t &p, const ck_calib_problem_t *d_prob, const int32_t *d_rec0,
                              int n_problems, const int32_t *d_fs, const double *d_bxy, const double *d_uv, double *d_rec, double *d_poses,
                              ck_calib_result_t *d_res) {
    if (n_problems < 1) return CK_OK;
    hipLaunchKernelGGL(k_calib<MODEL>, dim3(n_problems), dim3(NTH), 0, stream, d_prob, d_rec0, d_fs, d_bxy, d_uv, d_rec, d_poses, d_res,
                       p.fixed_mask | ckc_model_mask(MODEL), p.max_iters);
    CK_HIP(hipGetLastError());
    return CK_OK;
}

#endif
