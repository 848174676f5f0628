// k_rig_refine.hip — the maximum-likelihood refinement of the fused rig pose and its covariance: one 64-lane wave per
// instant, one wave per workgroup, the whole Levenberg-Marquardt iteration inside the kernel.  The solve is ck_rig_refine_math.h's, the
// same text the host twin (ck_rig_refine_host.c) compiles; this file only decides who computes what:
//   point records  lane l writes the records of the used points l, l + 64, ... of its instant (world corner, bearing, mount, camera) into
//                  the call's workspace once, and every later pass reads them back: a lane only ever reads what it wrote itself, so
//                  the wave needs no fence and no barrier
//   sums           lane l adds its points in index order; the 64 partial sums meet in the xor butterfly 32 .. 1 (__shfl_xor), which
//                  stands OUTSIDE the lanes' loops: every lane is active at every exchange, and every lane ends with the same bytes
//   small solves   the 6 x 6 (or 3 x 3) factorisation, the damping and the stop rules run in every lane on those same bytes: the
//                  control flow of the iteration is uniform without a broadcast
// No LDS, no private segment: every local array is indexed by constants once the loops are unrolled.  Plain C++ and __shfl_xor only.
#include "ck_rig_refine.h"
#include "ck_rig_refine_math.h"

namespace {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = CKF_LANES / 2; m >= 1; m >>= 1) v = v + __shfl_xor(v, m);
    return v;
}

__device__ __forceinline__ void load_point(const ckf_ctx_t *cx, int i, double *X, double *v, double *M) {
    const double *p = cx->pts + i;
#pragma unroll
    for (int k = 0; k < 3; k++) { X[k] = p[(size_t)k * cx->stride]; v[k] = p[(size_t)(3 + k) * cx->stride]; }
#pragma unroll
    for (int k = 0; k < 12; k++) M[k] = p[(size_t)(6 + k) * cx->stride];
}

} // namespace

CKC_FN void ckf_walk_jac(const ckf_ctx_t *cx, const int planar, const double *P, const double *xy, double *acc) {
    const int n = planar ? 9 : CKF_NSUM;
#pragma unroll
    for (int j = 0; j < n; j++) acc[j] = 0.0;
    for (int i = cx->lane; i < cx->np; i += CKF_LANES) {
        double X[3], v[3], M[12];
        load_point(cx, i, X, v, M);
        ckf_point_sums(planar, M, P, xy, X, v, acc);
    }
#pragma unroll
    for (int j = 0; j < n; j++) acc[j] = wave_sum(acc[j]);
}

CKC_FN void ckf_walk_cost(const ckf_ctx_t *cx, const double *P, double *cost, int *behind) {
    double a = 0.0;
    int bad = 0;
    for (int i = cx->lane; i < cx->np; i += CKF_LANES) {
        double X[3], v[3], M[12], e[3];
        load_point(cx, i, X, v, M);
        if (!(ckf_residual(M, P, X, v, e) > 0.0)) bad = 1;
        a = a + ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
    }
    *cost = wave_sum(a);
    *behind = __any(bad);
}

CKC_FN void ckf_walk_cams(const ckf_ctx_t *cx, const double *P, double *cam_cost) {
#pragma unroll
    for (int c = 0; c < CK_RIG_MAX_CAMS; c++) cam_cost[c] = 0.0;
    for (int i = cx->lane; i < cx->np; i += CKF_LANES) {
        double X[3], v[3], M[12], e[3];
        load_point(cx, i, X, v, M);
        ckf_residual(M, P, X, v, e);
        const int cam = (int)cx->pts[(size_t)18 * cx->stride + i];
#pragma unroll
        for (int c = 0; c < CK_RIG_MAX_CAMS; c++) // (an accumulator indexed by the camera would live in private memory)
            if (cam == c) cam_cost[c] = cam_cost[c] + ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
    }
#pragma unroll
    for (int c = 0; c < CK_RIG_MAX_CAMS; c++) cam_cost[c] = wave_sum(cam_cost[c]);
}

namespace {

__global__ __launch_bounds__(CKF_LANES) void k_rig_refine(const ck_rig_refine_args a) {
    const int s = blockIdx.x, lane = threadIdx.x;
    ck_rig_refined_t r = {};
    const ck_rig_result_t *st = reinterpret_cast<const ck_rig_result_t *>(a.start + (size_t)s * a.start_stride);
    if (!st->valid) {
        r.status = CK_RIG_REFINE_NO_START;
        if (lane == 0) a.out[s] = r;
        return;
    }
    // the instant's cameras: tags, masks, and where each camera's used points start
    int base[CK_RIG_MAX_CAMS + 1], nt[CK_RIG_MAX_CAMS], cam_np[CK_RIG_MAX_CAMS];
    uint64_t rej[CK_RIG_MAX_CAMS];
    base[0] = 0;
#pragma unroll
    for (int c = 0; c < CK_RIG_MAX_CAMS; c++) {
        nt[c] = 0; rej[c] = 0; cam_np[c] = 0;
        if (c < a.n_cams) {
            const int t = a.cam[c].problems[s].n_tags, cap = a.cam[c].det_cap;
            if (t > 0 && (cap == 0 || t <= cap)) {
                nt[c] = t;
                if (a.rejected) rej[c] = a.rejected[(size_t)s * a.rejected_stride + c];
                cam_np[c] = 4 * ckf_kept(t, rej[c]);
            }
        }
        base[c + 1] = base[c] + cam_np[c];
    }
    int np = base[CK_RIG_MAX_CAMS];
    if (np > a.max_points) { // (cannot happen: the workspace is sized from the same counts)
        np = 0;
#pragma unroll
        for (int c = 0; c < CK_RIG_MAX_CAMS; c++) cam_np[c] = 0;
    }
    double *pts = a.pts + (size_t)s * CKF_PT * (size_t)a.max_points;
    for (int i = lane; i < np; i += CKF_LANES) {
        int c = 0, b = 0, ntc = nt[0];
        uint64_t rj = rej[0];
        ck_rig_refine_cam cam = a.cam[0];
#pragma unroll
        for (int k = 1; k < CK_RIG_MAX_CAMS; k++)
            if (i >= base[k]) { c = k; b = base[k]; ntc = nt[k]; rj = rej[k]; cam = a.cam[k]; }
        const int j = i - b, t = ckf_kept_tag(ntc, rj, j >> 2), corner = j & 3;
        const ck_sqpnp_problem_t *p = cam.problems + s;
        const long long tag_at = cam.det_cap > 0 ? (long long)s * cam.det_cap : (long long)p->tag_offset;
        const long long bear_at = cam.det_cap > 0 ? (long long)s * cam.det_cap * 4 : (long long)p->bearing_offset;
        const ck_iso3_t *tag = cam.tags + tag_at + t;
        const double *v = cam.bearings + 3 * (bear_at + 4 * (long long)t + corner);
        double tt[3], tq[4], vv[3], bt[3], bq[4], rec[CKF_PT];
#pragma unroll
        for (int k = 0; k < 3; k++) { tt[k] = tag->t[k]; vv[k] = v[k]; bt[k] = p->robot_to_cam.t[k]; }
#pragma unroll
        for (int k = 0; k < 4; k++) { tq[k] = tag->q[k]; bq[k] = p->robot_to_cam.q[k]; }
        ckf_point_record(tt, tq, corner, vv, bt, bq, rec);
        rec[18] = (double)c;
#pragma unroll
        for (int k = 0; k < CKF_PT; k++) pts[(size_t)k * a.max_points + i] = rec[k];
    }
    const int prior = a.prm.gyro_sigma_rad > 0.0;
    double cg = 0.0, sg = 0.0;
    if (prior) {
        if (a.device_heading) { cg = cos(a.gyro[s]); sg = sin(a.gyro[s]); }
        else { cg = a.gyro[2 * (size_t)s]; sg = a.gyro[2 * (size_t)s + 1]; }
    }
    double rot0[9], pos0[3];
#pragma unroll
    for (int i = 0; i < 9; i++) rot0[i] = st->rot[i];
#pragma unroll
    for (int i = 0; i < 3; i++) pos0[i] = st->pos[i];
    const ckf_ctx_t cx = {pts, (size_t)a.max_points, np, lane, nullptr};
    if (a.prm.mode == CK_RIG_REFINE_PLANAR)
        ckf_solve(&cx, 1, a.prm.sigma_rad, a.prm.gyro_sigma_rad, a.prm.z, a.prm.max_iters, prior, cg, sg, rot0, pos0, cam_np, &r);
    else
        ckf_solve(&cx, 0, a.prm.sigma_rad, a.prm.gyro_sigma_rad, a.prm.z, a.prm.max_iters, prior, cg, sg, rot0, pos0, cam_np, &r);
    if (lane == 0) {
        a.out[s] = r;
        if (a.meas && r.status <= CK_RIG_REFINE_MAXITERS) {
            ck_vision_measurement_t *m = a.meas + s;
            m->pose_x = r.pos[0]; m->pose_y = r.pos[1]; m->pose_rot = atan2(r.rot[3], r.rot[0]);
            m->std_x = r.std_devs[0]; m->std_y = r.std_devs[1]; m->std_rot = r.std_devs[2];
        }
    }
}

} // namespace

int ck_launch_rig_refine(hipStream_t stream, const ck_rig_refine_args &a) {
    if (a.n < 1) return CK_OK;
    hipLaunchKernelGGL(k_rig_refine, dim3((unsigned)a.n), dim3(CKF_LANES), 0, stream, a);
    CK_HIP(hipGetLastError());
    return CK_OK;
}
