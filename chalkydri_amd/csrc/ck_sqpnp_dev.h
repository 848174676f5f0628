// ck_sqpnp_dev.h — the device pieces the two SQPnP kernels share: k_sqpnp (k_sqpnp.hip, one camera) and k_rig (k_rigpnp.hip, all the
// cameras of a robot) and that only a wave can run: the 16-lane SQP refinement, the wave-local Jacobi.  The arithmetic a single lane
// does, and the host twin with it, is ck_pose_math.h's.
#ifndef CK_SQPNP_DEV_H
#define CK_SQPNP_DEV_H

#include <math.h>

#include "ck_internal.h"
#include "ck_pose_math.h"

// One SQP refinement by a group of 16 lanes (lib.rs:98-115, 463-480): lane `gl` of the group owns one row of the
// 15x15 KKT system [[Omega, J^T], [J, 0]] in registers (lane 15 idles); r and the solution are replicated in every lane.
// LU with partial pivoting without moving rows: a lane remembers which logical row it holds (`lrow`), the pivot of a
// column is the unpivoted lane with the largest |entry| (smallest logical row on ties, like the sequential scan), its row
// is broadcast by shuffles and every other unpivoted lane eliminates in registers.  Each entry sees exactly the operations
// of the sequential code, in the same order, so the result is bit-identical to it.
// one step of an all-reduce over a DPP row (16 lanes): combine with the lane N places round the row (row_ror:N)
template <int N>
static __device__ __forceinline__ void row_max_step(double &best, int &meta) {
    const long long bits = __double_as_longlong(best);
    const int lo = __builtin_amdgcn_update_dpp((int)bits, (int)bits, 0x120 + N, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp((int)(bits >> 32), (int)(bits >> 32), 0x120 + N, 0xF, 0xF, false);
    const int om = __builtin_amdgcn_update_dpp(meta, meta, 0x120 + N, 0xF, 0xF, false);
    const double ob = __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
    if (ob > best || (ob == best && om < meta)) { best = ob; meta = om; }
}
// HAS_G: the cost has a linear term, E(r) = r^T Omega r - 2 g^T r + c (the rig solver), and the right-hand side is -(Omega r - g);
// without it `g` is never read and the step is SQPnP's own.  Returns r^T Omega r in both cases.
template <bool HAS_G>
static __device__ double optimization16(int max_iter, double tol_sq, double r[9], const double *omega, const double *g, int gl) {
    const int row = gl; // 0..14 own a row; 15 computes along on a zero row and is never a pivot
    for (int it = 0; it < max_iter; it++) {
        const double *c1 = r, *c2 = r + 3, *c3 = r + 6;
        double h[6];
        h[0] = c1[0] * c1[0] + c1[1] * c1[1] + c1[2] * c1[2] - 1.0;
        h[1] = c2[0] * c2[0] + c2[1] * c2[1] + c2[2] * c2[2] - 1.0;
        h[2] = c3[0] * c3[0] + c3[1] * c3[1] + c3[2] * c3[2] - 1.0;
        h[3] = c1[0] * c2[0] + c1[1] * c2[1] + c1[2] * c2[2];
        h[4] = c1[0] * c3[0] + c1[1] * c3[1] + c1[2] * c3[2];
        h[5] = c2[0] * c3[0] + c2[1] * c3[1] + c2[2] * c3[2];
        // J (6x9), rows: 0:(2c1,0,0) 1:(0,2c2,0) 2:(0,0,2c3) 3:(c2,c1,0) 4:(c3,0,c1) 5:(0,c3,c2)
        double J[6][9];
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int j = 0; j < 9; j++) J[i][j] = 0.0;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            J[0][k] = 2.0 * c1[k]; J[1][3 + k] = 2.0 * c2[k]; J[2][6 + k] = 2.0 * c3[k];
            J[3][k] = c2[k]; J[3][3 + k] = c1[k];
            J[4][k] = c3[k]; J[4][6 + k] = c1[k];
            J[5][3 + k] = c3[k]; J[5][6 + k] = c2[k];
        }
        double A[15], b = 0.0;
#pragma unroll
        for (int j = 0; j < 15; j++) A[j] = 0.0;
        if (row < 9) {
            double sacc = 0;
#pragma unroll
            for (int j = 0; j < 9; j++) { const double o = omega[row * 9 + j]; A[j] = o; sacc += o * r[j]; }
            if constexpr (HAS_G) b = -(sacc - g[row]); else b = -sacc;
#pragma unroll
            for (int i = 0; i < 6; i++) {
                double v = 0.0;
#pragma unroll
                for (int j = 0; j < 9; j++) v = (j == row) ? J[i][j] : v;
                A[9 + i] = v;
            }
        } else if (row < 15) {
#pragma unroll
            for (int i = 0; i < 6; i++)
                if (i == row - 9) {
#pragma unroll
                    for (int j = 0; j < 9; j++) A[j] = J[i][j];
                    b = -h[i];
                }
        }
        int lrow = row;          // logical row currently held by this lane
        bool pivoted = row >= 15; // lane 15 never takes part
        bool singular = false;
#pragma unroll
        for (int col = 0; col < 15; col++) {
            // pivot: largest |A[.][col]| among unpivoted lanes, smallest logical row on ties (the sequential scan keeps the
            // first maximum because it only replaces on a strictly larger value)
            // The 16 lanes of a group are one DPP row: four rotations (by 8, 4, 2, 1) with this combiner leave the same winner
            // in every lane — the order (value descending, logical row ascending) is total over the unpivoted lanes, so the
            // reduction order does not matter — and cost register moves instead of sixteen trips through the LDS crossbar.
            double best = pivoted ? -1.0 : fabs(A[col]);
            int meta = ((pivoted ? 99 : lrow) << 8) | gl; // logical row, then the lane that holds it
            row_max_step<8>(best, meta); row_max_step<4>(best, meta); row_max_step<2>(best, meta); row_max_step<1>(best, meta);
            const int bl = meta >> 8, bs = meta & 0xFF;
            if (best == 0.0) { singular = true; break; }
            // the lane that held logical row `col` takes over the pivot lane's logical row (a swap, without moving data)
            if (!pivoted && lrow == col && gl != bs) lrow = bl;
            const bool is_piv = gl == bs;
            if (is_piv) { lrow = col; }
            double P[15];
#pragma unroll
            for (int k = col; k < 15; k++) P[k] = __shfl(A[k], bs, 16);
            const double pb = __shfl(b, bs, 16);
            if (is_piv) pivoted = true;
            else if (!pivoted) {
                const double f = A[col] / P[col];
                if (f != 0.0) {
#pragma unroll
                    for (int k = col; k < 15; k++) A[k] -= f * P[k];
                    b -= f * pb;
                }
            }
        }
        if (singular) break;
        // back substitution over logical rows 14..0; the owner of a row finishes it and broadcasts the unknown
        double x[15];
#pragma unroll
        for (int rr = 14; rr >= 0; rr--) {
            double sv = b;
#pragma unroll
            for (int k = rr + 1; k < 15; k++) sv -= A[k] * x[k];
            sv = sv / A[rr];
            const unsigned long long own = __ballot(lrow == rr && gl < 15);
            const int src = (int)(__builtin_ctzll((own >> (threadIdx.x & 48)) & 0xFFFFull)); // owner inside this group of 16
            x[rr] = __shfl(sv, src, 16);
        }
        double n2 = 0;
#pragma unroll
        for (int k = 0; k < 9; k++) { r[k] += x[k]; n2 += x[k] * x[k]; }
        if (n2 < tol_sq) break;
    }
    double e = 0;
    for (int i = 0; i < 9; i++) {
        double sacc = 0;
        for (int j = 0; j < 9; j++) sacc += omega[i * 9 + j] * r[j];
        e += r[i] * sacc;
    }
    return e;
}

// Symmetric eigen-decomposition of the 9x9 in sA (destroyed: its diagonal holds the eigenvalues afterwards), eigenvectors in the
// columns of sV (the identity on entry), both in LDS: cyclic Jacobi, 9 lanes update one element of the rotated rows/columns.  The
// first wave does it alone (every lane of the workgroup may call; the others only compute the stop value): a wave's LDS accesses
// execute in program order, so the three hand-overs of a rotation need no workgroup barrier (36 rotations x ~10 sweeps x 3 barriers
// were a third of k_sqpnp's dependency chain).  The caller puts a workgroup barrier before and after.
static __device__ __forceinline__ void jacobi9_wave(double *sA, double *sV, int lane) {
    auto wave_sync = [] {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    double jtot = 0; // Frobenius norm^2 of Omega: the sweeps stop at 1e-32 of it (oracle: jacobi_eigen)
    for (int e = 0; e < 81; e++) jtot += sA[e] * sA[e];
    const double jstop = 1e-32 * jtot;
    if (lane < 64)
    for (int sweep = 0; sweep < 64; sweep++) {
        double off = 0;
        for (int i = 0; i < 9; i++)
            for (int j = i + 1; j < 9; j++) off += sA[i * 9 + j] * sA[i * 9 + j];
        if (off <= jstop) break;
        for (int p = 0; p < 9; p++)
            for (int q = p + 1; q < 9; q++) {
                double apq = sA[p * 9 + q];
                if (fabs(apq) < 1e-300) continue; // uniform: every lane reads the same LDS value
                double app = sA[p * 9 + p], aqq = sA[q * 9 + q];
                double theta = (aqq - app) / (2.0 * apq);
                double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                wave_sync();
                if (lane < 9) { int k = lane; double akp = sA[k * 9 + p], akq = sA[k * 9 + q]; sA[k * 9 + p] = c * akp - s * akq; sA[k * 9 + q] = s * akp + c * akq; }
                wave_sync();
                if (lane < 9) { int k = lane; double apk = sA[p * 9 + k], aqk = sA[q * 9 + k]; sA[p * 9 + k] = c * apk - s * aqk; sA[q * 9 + k] = s * apk + c * aqk; }
                if (lane < 9) { int k = lane; double vkp = sV[k * 9 + p], vkq = sV[k * 9 + q]; sV[k * 9 + p] = c * vkp - s * vkq; sV[k * 9 + q] = s * vkp + c * vkq; }
                wave_sync();
            }
    }
}

#endif
