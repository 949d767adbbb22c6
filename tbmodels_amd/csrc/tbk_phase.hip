// tbk_phase.hip -- phase-factor rows for one k-chunk.
//
// Reference step: the `np.exp(2j * np.pi * np.dot(k_array, R))` of
// /root/reference/src/tbmodels/_tb_model.py:1118, evaluated there once per stored R inside the
// Python loop.  Here every phase of a chunk is produced once, as two real rows per lattice vector:
//
//     A[2r    ][k] = cos(2 pi k.R_r)
//     A[2r + 1][k] = sin(2 pi k.R_r)          A is [k2][nk_pad], k contiguous
//
// which is the left operand of the real contraction in tbk_hk_dense.hip (its K index) and the
// gather table of tbk_hk_csr.hip.  k.R is accumulated in f64 with FMAs and handed to sincospi(2 k.R),
// whose argument reduction is exact, so |k| >> 1 costs no accuracy beyond the rounding of k.R itself
// (the reference multiplies by a rounded 2 pi first, which is worse).
//
// HBM-write bound: 16 B written per (k, R) against ~50 flops; one thread per (k, R), k fastest so a
// wave writes two 512 B row segments.

#include "tbk_internal.h"

namespace {

__global__ void __launch_bounds__(256)
phase_rows_kernel(const double* __restrict__ k, const int32_t* __restrict__ R, int dim, int64_t nk,
                  int64_t nk_pad, int64_t n_r, double* __restrict__ A) {
    const int64_t kidx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t r = blockIdx.y;
    if (kidx >= nk_pad) return;
    double c = 0.0, s = 0.0;
    if (kidx < nk && r < n_r) {
        double dot = 0.0;
        for (int d = 0; d < dim; ++d)
            dot = fma(k[kidx * dim + d], (double)R[r * dim + d], dot);
        sincospi(2.0 * dot, &s, &c);
    }
    A[(2 * r) * nk_pad + kidx] = c;
    A[(2 * r + 1) * nk_pad + kidx] = s;
}

// The rows of D^a = (1 / 2 pi) dH/dk_a (tbk_optics.hip): H = A B is real-linear in the phase rows, so the derivative is A' B with the same
// operand and A'[2r][k] = -R_a sin(2 pi k.R_r), A'[2r + 1][k] = +R_a cos(2 pi k.R_r) -- the arithmetic and the argument reduction of
// phase_rows_kernel, one more multiply.  Rows of R_a = 0 (R = 0 among them) and the padding are zeros.
__global__ void __launch_bounds__(256)
phase_rows_derivative_kernel(const double* __restrict__ k, const int32_t* __restrict__ R, int dim, int axis, int64_t nk,
                             int64_t nk_pad, int64_t n_r, double* __restrict__ A) {
    const int64_t kidx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t r = blockIdx.y;
    if (kidx >= nk_pad) return;
    double c = 0.0, s = 0.0;
    if (kidx < nk && r < n_r) {
        double dot = 0.0;
        for (int d = 0; d < dim; ++d)
            dot = fma(k[kidx * dim + d], (double)R[r * dim + d], dot);
        sincospi(2.0 * dot, &s, &c);
        const double ra = (double)R[r * dim + axis];
        const double ds = -(ra * s), dc = ra * c;
        c = ds;
        s = dc;
    }
    A[(2 * r) * nk_pad + kidx] = c;
    A[(2 * r + 1) * nk_pad + kidx] = s;
}

// The table of the left operands of one Strassen level (below), applied to quadrants v[k half][K half]
__device__ __forceinline__ void strassen_left(const double (&v)[2][2], double (&out)[7]) {
    out[0] = v[0][0] + v[1][1];
    out[1] = v[1][0] + v[1][1];
    out[2] = v[0][0];
    out[3] = v[1][1];
    out[4] = v[0][0] + v[0][1];
    out[5] = v[1][0] - v[0][0];
    out[6] = v[0][1] - v[1][1];
}

// The left operands of one Strassen level (tbk_hk_dense.hip).  P = A^T split into halves: k-points
// [0, Mh) | [Mh, 2 Mh), lattice vectors [0, n_r_pad / 2) | the rest; P_ab is k-half a x K-half b.  One thread per
// (k' < Mh, r' < n_r_pad / 2) forms the four quadrant phases with the arithmetic of phase_rows_kernel (k-points past nk and
// padding lattice vectors get cos = sin = 0) and writes the seven blocks As[7][K2 / 2][Mh], k contiguous:
//
//     As[0] = P11 + P22   As[1] = P21 + P22   As[2] = P11   As[3] = P22   As[4] = P11 + P12   As[5] = P21 - P11   As[6] = P12 - P22
__global__ void __launch_bounds__(256)
phase_rows_strassen_kernel(const double* __restrict__ k, const int32_t* __restrict__ R, int dim, int64_t nk, int64_t mh,
                           int64_t n_r, int64_t rh, double* __restrict__ As) {
    const int64_t kq = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t r = blockIdx.y;
    if (kq >= mh) return;
    double c[2][2], s[2][2];  // [k half][K half]
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int64_t kidx = kq + a * mh, rr = r + b * rh;
            c[a][b] = 0.0;
            s[a][b] = 0.0;
            if (kidx < nk && rr < n_r) {
                double dot = 0.0;
                for (int d = 0; d < dim; ++d) dot = fma(k[kidx * dim + d], (double)R[rr * dim + d], dot);
                sincospi(2.0 * dot, &s[a][b], &c[a][b]);
            }
        }
    const size_t blk = (size_t)2 * rh * mh;
#pragma unroll
    for (int t = 0; t < 2; ++t) {  // cos row 2r', sin row 2r' + 1
        double* row = As + (size_t)(2 * r + t) * mh + kq;
        double out[7];
        strassen_left(t == 0 ? c : s, out);
#pragma unroll
        for (int p = 0; p < 7; ++p) row[p * blk] = out[p];
    }
}

// Two levels: the table applied to each of its seven operands.  k-points and lattice vectors in QUARTERS (quarter 2 a1 + a2:
// half a1 of the outer split, half a2 of the inner one); one thread per (k' < Mq, r' < n_r_pad / 4) forms the 16 quadrant phases
// (padding k-points and lattice vectors: cos = sin = 0), the seven outer operands quadrant by quadrant, and of each the seven
// inner ones: As2[7 p1 + p2][K2 / 4][Mq], k contiguous -- 98 coalesced row segments per wave.  HBM-write bound.
__global__ void __launch_bounds__(256)
phase_rows_strassen2_kernel(const double* __restrict__ k, const int32_t* __restrict__ R, int dim, int64_t nk, int64_t mq,
                            int64_t n_r, int64_t rq, double* __restrict__ As2) {
    const int64_t kq = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t r = blockIdx.y;
    if (kq >= mq) return;
    double cs[2][4][4];  // [cos | sin][k quarter][K quarter]
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int64_t kidx = kq + a * mq, rr = r + b * rq;
            double c = 0.0, s = 0.0;
            if (kidx < nk && rr < n_r) {
                double dot = 0.0;
                for (int d = 0; d < dim; ++d) dot = fma(k[kidx * dim + d], (double)R[rr * dim + d], dot);
                sincospi(2.0 * dot, &s, &c);
            }
            cs[0][a][b] = c;
            cs[1][a][b] = s;
        }
    const size_t blk = (size_t)2 * rq * mq;
#pragma unroll
    for (int t = 0; t < 2; ++t) {  // cos row 2r', sin row 2r' + 1
        double* row = As2 + (size_t)(2 * r + t) * mq + kq;
        double outer[2][2][7];  // [inner k half][inner K half][p1]
#pragma unroll
        for (int a2 = 0; a2 < 2; ++a2)
#pragma unroll
            for (int b2 = 0; b2 < 2; ++b2) {
                const double v[2][2] = {{cs[t][a2][b2], cs[t][a2][2 + b2]}, {cs[t][2 + a2][b2], cs[t][2 + a2][2 + b2]}};
                strassen_left(v, outer[a2][b2]);
            }
#pragma unroll
        for (int p1 = 0; p1 < 7; ++p1) {
            const double v[2][2] = {{outer[0][0][p1], outer[0][1][p1]}, {outer[1][0][p1], outer[1][1][p1]}};
            double inner[7];
            strassen_left(v, inner);
#pragma unroll
            for (int p2 = 0; p2 < 7; ++p2) row[(size_t)(7 * p1 + p2) * blk] = inner[p2];
        }
    }
}

// k.p monomials (kdotp.py:71-78): A[p][k] = prod_d k_d^powers[p][d]
__global__ void __launch_bounds__(256)
monomial_rows_kernel(const double* __restrict__ k, const int32_t* __restrict__ powers, int dim,
                     int64_t nk, int64_t nk_pad, int64_t n_p, double* __restrict__ A) {
    const int64_t kidx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t p = blockIdx.y;
    if (kidx >= nk_pad) return;
    double v = 0.0;
    if (kidx < nk && p < n_p) {
        v = 1.0;
        for (int d = 0; d < dim; ++d) {
            const double x = k[kidx * dim + d];
            const int e = powers[p * dim + d];
            // repeated multiplication in increasing order, like numpy's integer power for small e
            double acc = 1.0;
            for (int t = 0; t < e; ++t) acc *= x;
            v *= acc;
        }
    }
    A[p * nk_pad + kidx] = v;
}

// convention 1 (_tb_model.py:1124-1128): e[k][p] = exp(2 pi i k.pos_p), one (cos, sin) pair per (k, orbital)
__global__ void __launch_bounds__(256)
orbital_phase_kernel(const double* __restrict__ k, const double* __restrict__ pos, int dim, int64_t nk,
                     int n_orb, double* __restrict__ orb) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nk * n_orb) return;
    const int64_t kq = idx / n_orb;
    const int p = (int)(idx % n_orb);
    double dot = 0.0;
    for (int d = 0; d < dim; ++d) dot = fma(k[kq * dim + d], pos[p * dim + d], dot);
    double s, c;
    sincospi(2.0 * dot, &s, &c);
    orb[2 * idx] = c;
    orb[2 * idx + 1] = s;
}

}  // namespace

int tbk_launch_orbital_phases(tbk_model* m, const double* d_k, const double* d_pos, int64_t nk, double* d_orb) {
    if (nk == 0) return TBK_OK;
    const int64_t total = nk * m->n_orb;
    hipLaunchKernelGGL(orbital_phase_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, m->stream, d_k,
                       d_pos, m->dim, nk, m->n_orb, d_orb);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

int tbk_launch_phase(tbk_model* m, const tbk_operand_t& op, const double* d_k, int64_t nk, int64_t nk_pad, double* d_A) {
    if (op.n_r_pad == 0 || nk_pad == 0) return TBK_OK;
    StageTimer t(m, TBK_T_PHASE);
    dim3 grid((unsigned)((nk_pad + 255) / 256), (unsigned)op.n_r_pad);
    hipLaunchKernelGGL(phase_rows_kernel, grid, dim3(256), 0, m->stream, d_k, op.d_R, op.dim, nk,
                       nk_pad, op.n_r, d_A);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

int tbk_launch_phase_derivative(tbk_model* m, const tbk_operand_t& op, const double* d_k, int64_t nk, int64_t nk_pad, int axis, double* d_A) {
    if (op.n_r_pad == 0 || nk_pad == 0) return TBK_OK;
    StageTimer t(m, TBK_T_PHASE);
    dim3 grid((unsigned)((nk_pad + 255) / 256), (unsigned)op.n_r_pad);
    hipLaunchKernelGGL(phase_rows_derivative_kernel, grid, dim3(256), 0, m->stream, d_k, op.d_R, op.dim, axis, nk, nk_pad, op.n_r, d_A);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

int tbk_launch_phase_strassen(tbk_model* m, const tbk_operand_t& op, const double* d_k, int64_t nk, double* d_As) {
    const int64_t mh = tbk_strassen_mh(nk), rh = op.n_r_pad / 2;
    StageTimer t(m, TBK_T_PHASE);
    dim3 grid((unsigned)((mh + 255) / 256), (unsigned)rh);
    hipLaunchKernelGGL(phase_rows_strassen_kernel, grid, dim3(256), 0, m->stream, d_k, op.d_R, op.dim, nk, mh, op.n_r, rh, d_As);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

int tbk_launch_phase_strassen2(tbk_model* m, const tbk_operand_t& op, const double* d_k, int64_t nk, double* d_As2) {
    const int64_t mq = tbk_strassen_mq(nk), rq = op.n_r_pad / 4;
    StageTimer t(m, TBK_T_PHASE);
    dim3 grid((unsigned)((mq + 255) / 256), (unsigned)rq);
    hipLaunchKernelGGL(phase_rows_strassen2_kernel, grid, dim3(256), 0, m->stream, d_k, op.d_R, op.dim, nk, mq, op.n_r, rq, d_As2);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

int tbk_launch_monomials(hipStream_t s, const int32_t* d_powers, int dim, int64_t n_p,
                         int64_t n_p_pad, const double* d_k, int64_t nk, int64_t nk_pad,
                         double* d_A) {
    if (n_p_pad == 0 || nk_pad == 0) return TBK_OK;
    dim3 grid((unsigned)((nk_pad + 255) / 256), (unsigned)n_p_pad);
    hipLaunchKernelGGL(monomial_rows_kernel, grid, dim3(256), 0, s, d_k, d_powers, dim, nk, nk_pad,
                       n_p, d_A);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}
