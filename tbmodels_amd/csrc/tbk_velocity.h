// tbk_velocity.h -- the rotation of D^a = (1 / 2 pi) dH/dk_a into the band basis, V^a = U^H D^a U, as tbk_optics.hip (the Kubo
// conductivity) and tbk_tdf.hip (the transport distribution, section 30) both run it: the swizzled planes of a
// staged matrix, the staging loop, the MFMA product of two staged matrices, and the library's two products above 64 orbitals.  Device
// code in an unnamed namespace: each translation unit instantiates its own, as with tbk_pair.h and tbk_zmfma.h.
//
// A matrix of up to NP x NP complex numbers (NP = 16, 32, 64, zeros beyond n) is staged as two planes Re / Im of NP x NP doubles in
// LDS.  Rows of 32 or 64 doubles are stored with column c ^ 16 in the odd rows, so that the two rows a ds_read_b64 group of 32 lanes
// reads land in different halves of the banks.
#pragma once

#include <algorithm>

#include "tbk_zmfma.h"

namespace {

constexpr int OPT_FUSED_MAX = 64;  // orbitals of the fused kernels, at most

// the place of element (row o, column c) in a plane of NP x NP doubles
template <int NP>
__device__ __forceinline__ int opt_at(int o, int c) {
    return o * NP + (NP == 16 ? c : c ^ ((o & 1) << 4));
}

// (cr, ci) += X^H Y for the wave's tile row ti and tiles tj0 ... tj0 + TPW - 1: `steps` MFMA steps of four rows of the planes
template <int NP, int TPW>
__device__ __forceinline__ void opt_product(const double* __restrict__ xr, const double* __restrict__ xi, const double* __restrict__ yr,
                                            const double* __restrict__ yi, int steps, int ti, int tj0, int lane, zd4 (&cr)[TPW], zd4 (&ci)[TPW]) {
    const int l15 = lane & 15, lq = lane >> 4;
#pragma unroll 1
    for (int s = 0; s < steps; ++s) {
        const int o = 4 * s + lq;
        const int ia = opt_at<NP>(o, ti * 16 + l15);
        const double ar = xr[ia], ai = xi[ia];
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
            const int ib = opt_at<NP>(o, (tj0 + t) * 16 + l15);
            const double br = yr[ib], bi = yi[ib];
            zmfma_ahb(ar, ai, br, bi, cr[t], ci[t]);
        }
    }
}

// the n x n matrix M (row-major) into the planes (pr, pi) by the TEAM threads of one k-point, thread tt of them; zeros beyond n and
// without `valid`
template <int NP, int TEAM>
__device__ __forceinline__ void opt_stage(const double2* M, int n, bool valid, int tt, double* pr, double* pi) {
    for (int idx = tt; idx < NP * NP; idx += TEAM) {
        const int o = idx / NP, c = idx - o * NP;
        double2 v = make_double2(0.0, 0.0);
        if (valid && o < n && c < n) v = M[(size_t)o * n + c];
        pr[opt_at<NP>(o, c)] = v.x;
        pi[opt_at<NP>(o, c)] = v.y;
    }
}

// The library route's two products of nb k-points and one axis on row-major matrices, which the library reads as their transposes:
// V^T = U^T D^T conj(U), so with Uc, Dc the library's views T = Dc Uc^H and Vc = Uc T; V^a takes D^a's place (stride d_sk complex
// numbers between the k-points), T[nb][n][n] is scratch.
inline int opt_library_rotate(rocblas_handle blas, int n, rocblas_int nb, const rocblas_double_complex* Uc, rocblas_double_complex* Da, size_t d_sk,
                              rocblas_double_complex* Tc) {
    const rocblas_double_complex one(1.0, 0.0), zero(0.0, 0.0);
    const int64_t nn = (int64_t)n * n;
    TBK_ROCBLAS(rocblas_zgemm_strided_batched(blas, rocblas_operation_none, rocblas_operation_conjugate_transpose, n, n, n, &one, Da, n,
                                              (rocblas_stride)d_sk, Uc, n, (rocblas_stride)nn, &zero, Tc, n, (rocblas_stride)nn, nb));
    TBK_ROCBLAS(rocblas_zgemm_strided_batched(blas, rocblas_operation_none, rocblas_operation_none, n, n, n, &one, Uc, n, (rocblas_stride)nn, Tc, n,
                                              (rocblas_stride)nn, &zero, Da, n, (rocblas_stride)d_sk, nb));
    return TBK_OK;
}

}  // namespace
