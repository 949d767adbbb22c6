// tbk_stage.hip -- one-time staging of the hoppings into the layout the H(k) kernel contracts.
//
// The reference walks `self.hop` (dict R -> N x N complex) on every call
// (/root/reference/src/tbmodels/_tb_model.py:1111) and adds the Hermitian conjugate afterwards
// (:1123).  Because H = A + A^H is real-linear in (cos, sin) of each phase, the conjugate part can
// be folded into the staged operand ONCE, and only the upper triangle i <= j is ever contracted:
//
//     H[i][j] = sum_R  p_R h_R[i][j] + conj(p_R) conj(h_R[j][i]),      p_R = c_R + i s_R
//     Re H[i][j] = sum_R  c_R (hr_ij + hr_ji)  -  s_R (hi_ij + hi_ji)
//     Im H[i][j] = sum_R  c_R (hi_ij - hi_ji)  +  s_R (hr_ij - hr_ji)
//
// i.e. a REAL contraction  H[k][e] = sum_kk A[kk][k] * B[kk][e]  with two K rows per lattice vector
// (kk = 2r: cos, kk = 2r+1: sin) and two real output columns (Re, Im) per packed element e = (i <= j).
// That halves the flops of the straightforward complex contraction (N(N+1)/2 instead of N^2 complex
// columns) and removes the transpose-add pass.  Diagonal elements get Im == 0 exactly, as in the
// reference.
//
// Their Re columns are all that is contracted for diagonal elements: a dense model puts two of them in one slot
// (TBK_SLOT_PAIR, tbk_internal.h), cos row (2 hr_ii | 2 hr_jj), sin row (-2 hi_ii | -2 hi_jj) -- the very values the
// single-element slot holds in its Re plane, so each column's arithmetic is unchanged.  At N_orb = 64 that is 2048
// slots (32 element tiles) instead of 2080 padded to 2112 (33 tiles).  k.p models keep one slot per element (the Im
// of their diagonal is the caller's).
//
// Layout written here ("tile-interleaved", so one workgroup row segment is contiguous):
//
//     Bt[kk][e / 16][plane][e % 16]      plane 0 = Re column, 1 = Im column (pair slot: Re of H[j][j]); f64
//
// Padding rows (r >= n_r) and padding elements (e >= ncol) are zero.

#include "tbk_internal.h"

namespace {

__global__ void __launch_bounds__(256)
stage_dense_kernel(const double* __restrict__ hop, const int32_t* __restrict__ colmap, int n_orb,
                   int64_t n_r, int ncol_pad, double* __restrict__ Bt) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t r = blockIdx.y;
    if (e >= ncol_pad || r >= n_r) return;
    const int32_t ij = colmap[e];
    if (ij < 0) return;
    const int i = ij >> 16, j = ij & 0x7fff;
    const double* blk = hop + (size_t)r * n_orb * n_orb * 2;
    const size_t tiles = ncol_pad / TBK_CT;
    const size_t base0 = (((size_t)(2 * r) * tiles + e / TBK_CT) * 2) * TBK_CT + e % TBK_CT;
    const size_t base1 = (((size_t)(2 * r + 1) * tiles + e / TBK_CT) * 2) * TBK_CT + e % TBK_CT;
    if (ij & TBK_SLOT_PAIR) {  // H[i][i] in plane 0, H[j][j] in plane 1
        const double hr = blk[((size_t)i * n_orb + i) * 2], hi = blk[((size_t)i * n_orb + i) * 2 + 1];
        const double gr = blk[((size_t)j * n_orb + j) * 2], gi = blk[((size_t)j * n_orb + j) * 2 + 1];
        Bt[base0] = hr + hr;
        Bt[base0 + TBK_CT] = gr + gr;
        Bt[base1] = -(hi + hi);
        Bt[base1 + TBK_CT] = -(gi + gi);
        return;
    }
    const double hr = blk[((size_t)i * n_orb + j) * 2], hi = blk[((size_t)i * n_orb + j) * 2 + 1];
    const double gr = blk[((size_t)j * n_orb + i) * 2], gi = blk[((size_t)j * n_orb + i) * 2 + 1];
    Bt[base0] = hr + gr;              // cos row, Re column
    Bt[base0 + TBK_CT] = hi - gi;     // cos row, Im column
    Bt[base1] = -(hi + gi);           // sin row, Re column
    Bt[base1 + TBK_CT] = hr - gr;     // sin row, Im column
}

// k.p coefficients: one real K row per monomial, H[e] = sum_p mono_p * C_p[i][j]
__global__ void __launch_bounds__(256)
stage_kdotp_kernel(const double* __restrict__ coeff, const int32_t* __restrict__ colmap, int n_orb,
                   int64_t n_p, int ncol_pad, double* __restrict__ Bt) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t p = blockIdx.y;
    if (e >= ncol_pad || p >= n_p) return;
    const int32_t ij = colmap[e];
    if (ij < 0) return;
    const int i = ij >> 16, j = ij & 0xffff;
    const double* blk = coeff + (size_t)p * n_orb * n_orb * 2;
    const size_t tiles = ncol_pad / TBK_CT;
    const size_t base = (((size_t)p * tiles + e / TBK_CT) * 2) * TBK_CT + e % TBK_CT;
    Bt[base] = blk[((size_t)i * n_orb + j) * 2];
    Bt[base + TBK_CT] = blk[((size_t)i * n_orb + j) * 2 + 1];
}

// One Strassen level (tbk_hk_dense.hip): the right operand of product p is a sum of the quadrants
// B_bc = Bt[b-th half of K][c-th half of the slots] -- in the tile-interleaved layout a slot half is one contiguous half of
// every K row, so each block is an ordinary operand of ncol_pad / 2 slots:
//
//     Bs[0] = B11 + B22   Bs[1] = B11   Bs[2] = B12 - B22   Bs[3] = B21 - B11   Bs[4] = B22   Bs[5] = B11 + B12   Bs[6] = B21 + B22
//
// One thread per (K row of the half, double of the half row).
__global__ void __launch_bounds__(256)
stage_strassen_kernel(const double* __restrict__ Bt, int64_t kh, int ncol_pad, double* __restrict__ Bs) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;  // < ncol_pad: a half row holds ncol_pad / 2 slots x 2 planes
    const int64_t kk = blockIdx.y;
    if (j >= ncol_pad) return;
    const size_t row = (size_t)2 * ncol_pad;
    const double b11 = Bt[kk * row + j], b12 = Bt[kk * row + ncol_pad + j];
    const double b21 = Bt[(kk + kh) * row + j], b22 = Bt[(kk + kh) * row + ncol_pad + j];
    const size_t blk = (size_t)kh * ncol_pad, o = kk * (size_t)ncol_pad + j;
    Bs[0 * blk + o] = b11 + b22;
    Bs[1 * blk + o] = b11;
    Bs[2 * blk + o] = b12 - b22;
    Bs[3 * blk + o] = b21 - b11;
    Bs[4 * blk + o] = b22;
    Bs[5 * blk + o] = b11 + b12;
    Bs[6 * blk + o] = b21 + b22;
}

}  // namespace

// The Strassen operand blocks of a dense model padded for them (tbk_api.hip create_common).  7/4 of Bt; a model whose blocks
// would take more than a quarter of the free HBM keeps the classical path only (d_Bs stays NULL).
int tbk_stage_strassen(tbk_model* m) {
    if (!tbk_strassen_model(m->sparse, m->kdotp, m->n_r) || m->d_B == nullptr) return TBK_OK;
    const int64_t kh = m->k2 / 2;
    if (kh % TBK_BK != 0 || m->ncol_pad % (2 * TBK_BNP) != 0 || kh > 65535) return TBK_OK;
    const size_t bytes = (size_t)7 * kh * m->ncol_pad * sizeof(double);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || bytes > free_b / 4) return TBK_OK;
    TBK_HIP(hipMalloc(m->d_Bs.put(), bytes));
    m->staged_bytes += (int64_t)bytes;
    dim3 grid((m->ncol_pad + 255) / 256, (unsigned)kh);
    hipLaunchKernelGGL(stage_strassen_kernel, grid, dim3(256), 0, m->stream, m->d_B, kh, m->ncol_pad, m->d_Bs);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

// The blocks of the second level: Bs2[7 p1 + p2] is the table applied to the quadrants of Bs[p1] -- K halves of K2 / 4 rows, slot
// halves of ncol_pad / 4 slots, contiguous in every row like the halves of Bt -- i.e. stage_strassen_kernel on each of the seven
// blocks: the inner table applied to the outer table's operands, every sum in a fixed order.  49/16 of Bt, not built with the
// model: most models never run a chunk long enough to read them (choose_chunk decides, fill_rows calls this).
size_t tbk_strassen2_bytes(const tbk_model* m) { return (size_t)49 * (m->k2 / 4) * (m->ncol_pad / 2) * sizeof(double); }

int tbk_stage_strassen2(tbk_model* m) {
    if (m->d_Bs2 != nullptr) return TBK_OK;
    TBK_ARG(m->d_Bs != nullptr && m->k2 % (4 * TBK_BK) == 0 && m->ncol_pad % (4 * TBK_BNP) == 0, "model is not staged for two Strassen levels");
    const int64_t kq = m->k2 / 4;
    const int half = m->ncol_pad / 2;
    const size_t bytes = tbk_strassen2_bytes(m);
    TBK_HIP(hipMalloc(m->d_Bs2.put(), bytes));
    m->staged_bytes += (int64_t)bytes;
    const size_t blk1 = (size_t)2 * kq * m->ncol_pad, blk2 = (size_t)kq * half;  // doubles per block of Bs, of Bs2
    for (int p1 = 0; p1 < 7; ++p1) {
        dim3 grid((half + 255) / 256, (unsigned)kq);
        hipLaunchKernelGGL(stage_strassen_kernel, grid, dim3(256), 0, m->stream, m->d_Bs + p1 * blk1, kq, half, m->d_Bs2 + 7 * p1 * blk2);
        TBK_HIP(hipGetLastError());
    }
    return TBK_OK;
}

int tbk_stage_dense(tbk_model* m, const double* d_hop_raw) {
    const size_t bytes = (size_t)m->k2 * m->ncol_pad * 2 * sizeof(double);
    if (bytes == 0) return TBK_OK;
    TBK_HIP(hipMalloc(m->d_B.put(), bytes));
    m->staged_bytes += (int64_t)bytes;
    TBK_HIP(hipMemsetAsync(m->d_B, 0, bytes, m->stream));
    if (m->n_r > 0) {
        TBK_ARG(m->n_r <= 65535, "more than 65535 lattice vectors");
        dim3 grid((m->ncol_pad + 255) / 256, (unsigned)m->n_r);
        hipLaunchKernelGGL(stage_dense_kernel, grid, dim3(256), 0, m->stream, d_hop_raw, m->d_colmap,
                           m->n_orb, m->n_r, m->ncol_pad, m->d_B);
        TBK_HIP(hipGetLastError());
    }
    return TBK_OK;
}

int tbk_stage_kdotp(tbk_model* m, const double* d_coeff_raw) {
    const size_t bytes = (size_t)m->k2 * m->ncol_pad * 2 * sizeof(double);
    if (bytes == 0) return TBK_OK;
    TBK_HIP(hipMalloc(m->d_B.put(), bytes));
    m->staged_bytes += (int64_t)bytes;
    TBK_HIP(hipMemsetAsync(m->d_B, 0, bytes, m->stream));
    if (m->n_r > 0) {
        TBK_ARG(m->n_r <= 65535, "more than 65535 Taylor coefficients");
        dim3 grid((m->ncol_pad + 255) / 256, (unsigned)m->n_r);
        hipLaunchKernelGGL(stage_kdotp_kernel, grid, dim3(256), 0, m->stream, d_coeff_raw,
                           m->d_colmap, m->n_orb, m->n_r, m->ncol_pad, m->d_B);
        TBK_HIP(hipGetLastError());
    }
    return TBK_OK;
}
