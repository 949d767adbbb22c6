// tbk_eigh.hip -- eigenvalues AND eigenvectors of H(k): Model.eigh / KdotpModel.eigh.
//
// Per k chunk: the H(k) of the chunk is built (full matrix, the call's convention) straight into the chunk's rows of the
// output U, and one eigenvector launch overwrites every matrix with its eigenvectors in place -- no N^2 workspace.
//
//   n_orb <= 64 (AUTO, WAVE): jacobi_eigh_kernel, parallel cyclic two-sided Jacobi on the Hermitian matrix, the matrix A
//                             and the accumulated rotations V in LDS.
//   n_orb > 64 or ROCSOLVER:  rocsolver_zheev_strided_batched with rocblas_evect_original, then one small kernel that
//                             turns the column-major output around (eigh_finish_kernel).  (zheevd, the divide-and-conquer
//                             driver the eigenvalue path uses, returned NaN eigenvectors -- info 0 -- for test matrices of
//                             100 and 129 orbitals; the QR driver zheev is the one used here.)
//
// Jacobi.  The matrix is padded to NP in {8, 16, 32, 64}; a round-robin (tournament) ordering gives
// NP - 1 rounds per sweep of NP / 2 disjoint pairs each, and pairs that touch a padded index are skipped -- the padding never
// couples to the matrix, so it adds no eigenvalues.  The rotations of one round commute (disjoint pairs): the round is
// A <- G^H A G with G block-diagonal, applied as one pass over the rows p, q of every pair, then one over the columns p, q
// of A and V.  The pair (p, q) with a_pq = |a_pq| e^{i phi}, zeta = (a_qq - a_pp) / (2 |a_pq|):
//     t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)),  c = 1 / sqrt(1 + t^2),  s = t c,  se = s e^{i phi}
//     G = [[c, se], [-conj(se), c]]:  a_pp <- a_pp - t |a_pq|,  a_qq <- a_qq + t |a_pq|,  a_pq <- 0 exactly.
// A pair is skipped when |a_pq| <= eps sqrt(|a_pp| |a_qq|) -- the relative criterion that keeps Jacobi accurate on graded
// matrices -- and the kernel stops after the first sweep that rotates nothing (at most TBK_JACOBI_MAX_SWEEPS sweeps, then
// the no-convergence flag).  A matrix's arithmetic does not depend on the call: the same element-wise updates in the same
// order whatever the batch, no cross-matrix reduction.

#include <rocsolver/rocsolver.h>

#include <algorithm>
#include <cfloat>
#include <cstring>

#include "tbk_internal.h"

namespace {

constexpr int TBK_JACOBI_MAX_SWEEPS = 30;

// Matrices per workgroup and threads per matrix: NP^2 / 8 threads give every thread 4 (pair, column) items of the row pass
// and 4 (pair, row) items of A and of V in the column pass.  NP = 64 takes 130 KiB of LDS (one workgroup of 8 waves per
// CU); NP <= 32 ~66 - 72 KiB per workgroup of 4 waves (two per CU).
template <int NP>
struct JacobiShape {
    static constexpr int G = NP * NP / 8;               // threads per matrix
    static constexpr int MPB = NP == 64 ? 1 : 256 / G;  // matrices per workgroup
    static constexpr int T = G * MPB;                   // threads per workgroup
    static constexpr int LD = NP + 1;                   // LDS row stride (complex): column walks hit distinct banks
};

struct Cplx {
    double re, im;
};

template <int NP>
__global__ void __launch_bounds__(JacobiShape<NP>::T)
    jacobi_eigh_kernel(double* __restrict__ U, double* __restrict__ E, int n, int64_t nk, int* __restrict__ flag) {
    using S = JacobiShape<NP>;
    constexpr int G = S::G, MPB = S::MPB, LD = S::LD, NPAIR = NP / 2;
    __shared__ Cplx A[MPB][NP * LD];
    __shared__ Cplx Vt[MPB][NP * LD];  // Vt[j][i] = V[i][j]: a column of V is a row here
    __shared__ double rot_c[MPB][NPAIR], rot_sr[MPB][NPAIR], rot_si[MPB][NPAIR], rot_dp[MPB][NPAIR], rot_dq[MPB][NPAIR];
    __shared__ double row_max[MPB][NP];
    __shared__ int row_bad[MPB][NP];
    __shared__ int perm[MPB][NP];
    __shared__ int live[MPB];     // 1 while the matrix iterates
    __shared__ int rotated[MPB];  // the current sweep rotated something
    __shared__ int bad[MPB];      // non-finite input
    __shared__ double unscale[MPB];

    const int ml = threadIdx.x / G, lt = threadIdx.x % G;
    const int64_t mat = (int64_t)blockIdx.x * MPB + ml;
    const bool active = mat < nk;
    Cplx* a = A[ml];
    Cplx* vt = Vt[ml];
    double* H = U + (size_t)(active ? mat : 0) * n * n * 2;

    // load: the stored upper triangle, mirrored; padding 0; V = I
    for (int e = lt; e < NP * NP; e += G) {
        const int i = e / NP, j = e % NP;
        if (i >= n || j >= n || !active) a[i * LD + j] = Cplx{0.0, 0.0};
        vt[i * LD + j] = Cplx{i == j ? 1.0 : 0.0, 0.0};
        if (e < NP) perm[ml][e] = e;  // (every entry in range whatever the ranks below)
    }
    if (active)
        for (int e = lt; e < n * n; e += G) {
            const int i = e / n, j = e % n;
            if (j < i) continue;
            const double re = H[2 * (size_t)e], im = H[2 * (size_t)e + 1];
            if (i == j) {
                a[i * LD + i] = Cplx{re, 0.0};
            } else {
                a[i * LD + j] = Cplx{re, im};
                a[j * LD + i] = Cplx{re, -im};
            }
        }
    __syncthreads();
    // scale: max |h_ij| of the stored triangle to [1, 2) by an exact power of two (the rule of tbk_eig.hip scale_to_unit_kernel)
    for (int i = lt; i < NP; i += G) {
        double mx = 0.0;
        int nf = 0;
        if (active && i < n)
            for (int j = i; j < n; ++j) {
                const Cplx v = a[i * LD + j];
                nf |= !isfinite(v.re) || !isfinite(v.im);
                mx = fmax(mx, fmax(fabs(v.re), fabs(v.im)));
            }
        row_max[ml][i] = mx;
        row_bad[ml][i] = nf;
    }
    __syncthreads();
    if (lt == 0) {
        double mx = 0.0;
        int nf = 0;
        for (int i = 0; i < n; ++i) {
            mx = fmax(mx, row_max[ml][i]);
            nf |= row_bad[ml][i];
        }
        const double s = (mx > 0.0 && !nf) ? ldexp(1.0, -ilogb(mx)) : 1.0;
        unscale[ml] = 1.0 / s;
        row_max[ml][0] = s;
        bad[ml] = active ? nf : 0;
        live[ml] = active && !nf;
        rotated[ml] = 0;
        if (active && nf) atomicAdd(flag + 1, 1);
    }
    __syncthreads();
    {
        const double s = row_max[ml][0];
        if (s != 1.0)
            for (int e = lt; e < NP * NP; e += G) {
                const int i = e / NP, j = e % NP;
                a[i * LD + j].re *= s;
                a[i * LD + j].im *= s;
            }
    }
    __syncthreads();

    for (int sweep = 0; sweep < TBK_JACOBI_MAX_SWEEPS; ++sweep) {
        bool any = false;
        for (int m = 0; m < MPB; ++m) any |= live[m] != 0;
        if (!any) break;  // (uniform: every thread read the same flags after a barrier)
        const bool mine = live[ml] != 0;
        for (int r = 0; r < NP - 1; ++r) {
            // the rotations of this round's pairs
            for (int k = lt; k < NPAIR; k += G) {
                const int x = k == 0 ? NP - 1 : (r + k) % (NP - 1), y = k == 0 ? r : (r - k + NP - 1) % (NP - 1);
                const int p = min(x, y), q = max(x, y);
                double c = -1.0, sr = 0.0, si = 0.0, dp = 0.0, dq = 0.0;  // c < 0: no rotation
                if (mine && q < n) {
                    const double app = a[p * LD + p].re, aqq = a[q * LD + q].re;
                    const Cplx apq = a[p * LD + q];
                    const double beta = hypot(apq.re, apq.im);
                    if (beta > DBL_EPSILON * sqrt(fabs(app)) * sqrt(fabs(aqq))) {
                        const double zeta = (aqq - app) / (2.0 * beta);
                        const double az = fabs(zeta);
                        double t = az > 1e100 ? 0.5 / az : 1.0 / (az + sqrt(1.0 + az * az));
                        if (zeta < 0.0) t = -t;
                        c = 1.0 / sqrt(1.0 + t * t);
                        const double s = t * c;
                        sr = s * (apq.re / beta);
                        si = s * (apq.im / beta);
                        dp = app - t * beta;
                        dq = aqq + t * beta;
                        rotated[ml] = 1;
                    }
                }
                rot_c[ml][k] = c;
                rot_sr[ml][k] = sr;
                rot_si[ml][k] = si;
                rot_dp[ml][k] = dp;
                rot_dq[ml][k] = dq;
            }
            __syncthreads();
            // rows:  a_p. <- c a_p. - se a_q.,   a_q. <- conj(se) a_p. + c a_q.
            if (mine)
                for (int e = lt; e < NPAIR * NP; e += G) {
                    const int k = e / NP, j = e % NP;
                    const double c = rot_c[ml][k], sr = rot_sr[ml][k], si = rot_si[ml][k];
                    if (c < 0.0) continue;
                    const int x = k == 0 ? NP - 1 : (r + k) % (NP - 1), y = k == 0 ? r : (r - k + NP - 1) % (NP - 1);
                    const int p = min(x, y), q = max(x, y);
                    const Cplx u = a[p * LD + j], v = a[q * LD + j];
                    a[p * LD + j] = Cplx{c * u.re - (sr * v.re - si * v.im), c * u.im - (sr * v.im + si * v.re)};
                    a[q * LD + j] = Cplx{(sr * u.re + si * u.im) + c * v.re, (sr * u.im - si * u.re) + c * v.im};
                }
            __syncthreads();
            // columns of A and V:  x_.p <- c x_.p - conj(se) x_.q,   x_.q <- se x_.p + c x_.q;  the pair's 2 x 2 block exactly
            if (mine)
                for (int e = lt; e < NPAIR * NP; e += G) {
                    const int k = e / NP, i = e % NP;
                    const double c = rot_c[ml][k], sr = rot_sr[ml][k], si = rot_si[ml][k];
                    if (c < 0.0) continue;
                    const int x = k == 0 ? NP - 1 : (r + k) % (NP - 1), y = k == 0 ? r : (r - k + NP - 1) % (NP - 1);
                    const int p = min(x, y), q = max(x, y);
                    if (i == p) {
                        a[p * LD + p] = Cplx{rot_dp[ml][k], 0.0};
                        a[p * LD + q] = Cplx{0.0, 0.0};
                    } else if (i == q) {
                        a[q * LD + p] = Cplx{0.0, 0.0};
                        a[q * LD + q] = Cplx{rot_dq[ml][k], 0.0};
                    } else {
                        const Cplx u = a[i * LD + p], v = a[i * LD + q];
                        a[i * LD + p] = Cplx{c * u.re - (sr * v.re + si * v.im), c * u.im - (sr * v.im - si * v.re)};
                        a[i * LD + q] = Cplx{(sr * u.re - si * u.im) + c * v.re, (sr * u.im + si * u.re) + c * v.im};
                    }
                    const Cplx u = vt[p * LD + i], v = vt[q * LD + i];
                    vt[p * LD + i] = Cplx{c * u.re - (sr * v.re + si * v.im), c * u.im - (sr * v.im - si * v.re)};
                    vt[q * LD + i] = Cplx{(sr * u.re - si * u.im) + c * v.re, (sr * u.im + si * u.re) + c * v.im};
                }
            __syncthreads();
        }
        if (lt == 0) {
            if (!rotated[ml]) live[ml] = 0;  // a sweep without a rotation: converged
            rotated[ml] = 0;
        }
        __syncthreads();
    }
    if (lt == 0 && live[ml]) atomicAdd(flag, 1);  // still rotating after the last sweep

    // ascending order, ties by index (deterministic): perm[rank] = i
    for (int i = lt; i < n; i += G) {
        const double d = a[i * LD + i].re;
        int rank = bad[ml] ? i : 0;
        for (int j = 0; j < n && !bad[ml]; ++j) {
            const double dj = a[j * LD + j].re;
            rank += (dj < d || (dj == d && j < i)) ? 1 : 0;
        }
        perm[ml][rank] = i;
    }
    __syncthreads();
    if (!active) return;
    const bool nan_out = bad[ml] != 0;
    const double qnan = __builtin_nan("");
    for (int j = lt; j < n; j += G) {
        const int i = perm[ml][j];
        E[(size_t)mat * n + j] = nan_out ? qnan : a[i * LD + i].re * unscale[ml];
    }
    // U[r][j] = component r of eigenvector j = V[r][perm[j]]
    for (int e = lt; e < n * n; e += G) {
        const int r = e / n, j = e % n;
        const Cplx v = vt[perm[ml][j] * LD + r];
        H[2 * (size_t)e] = nan_out ? qnan : v.re;
        H[2 * (size_t)e + 1] = nan_out ? qnan : v.im;
    }
}

template <int NP>
int launch_jacobi(tbk_model* m, double* d_U, int64_t nk, double* d_E) {
    using S = JacobiShape<NP>;
    const int64_t blocks = (nk + S::MPB - 1) / S::MPB;
    hipLaunchKernelGGL(jacobi_eigh_kernel<NP>, dim3((unsigned)blocks), dim3(S::T), 0, m->stream, d_U, d_E, m->n_orb, nk,
                       m->ws_flag.as<int>());
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

// ---- rocSOLVER branch ------------------------------------------------------------------------------------------------
// One workgroup per matrix: max |h_ij| of the stored (row-major upper) triangle to [1, 2) by an exact power of two, as
// tbk_eig.hip scale_to_unit_kernel does.  A non-finite matrix is replaced by 0 (the library never sees NaN / Inf) and gets
// scale NaN, which eigh_finish_kernel turns into NaN output and the non-finite flag.
__global__ void __launch_bounds__(256) eigh_scale_kernel(double* __restrict__ H, int n, double* __restrict__ scale) {
    __shared__ double smax[4];
    __shared__ int sbad[4];
    double* A = H + (size_t)blockIdx.x * n * n * 2;
    const size_t count = (size_t)n * n;
    double mx = 0.0;
    int nf = 0;
    for (size_t i = threadIdx.x; i < count; i += 256) {
        const size_t r = i / n, c = i % n;
        if (c < r) continue;
        nf |= !isfinite(A[2 * i]) || !isfinite(A[2 * i + 1]);
        mx = fmax(mx, fmax(fabs(A[2 * i]), fabs(A[2 * i + 1])));
    }
    for (int off = 32; off > 0; off >>= 1) {
        mx = fmax(mx, __shfl_xor(mx, off, 64));
        nf |= __shfl_xor(nf, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        smax[threadIdx.x >> 6] = mx;
        sbad[threadIdx.x >> 6] = nf;
    }
    __syncthreads();
    mx = fmax(fmax(smax[0], smax[1]), fmax(smax[2], smax[3]));
    nf = sbad[0] | sbad[1] | sbad[2] | sbad[3];
    const double s = (mx > 0.0 && !nf) ? ldexp(1.0, -ilogb(mx)) : 1.0;
    if (nf || s != 1.0)
        for (size_t i = threadIdx.x; i < count; i += 256) {
            A[2 * i] = nf ? 0.0 : A[2 * i] * s;
            A[2 * i + 1] = nf ? 0.0 : A[2 * i + 1] * s;
        }
    if (threadIdx.x == 0) scale[blockIdx.x] = nf ? __builtin_nan("") : 1.0 / s;
}

// zheev read the row-major H as column-major, i.e. conj(H); its eigenvectors conj(u_j) are the columns of the buffer,
// i.e. its rows in row-major terms: U = buffer^H, transposed in place (one thread per pair (r, c), r <= c).  Eigenvalues
// are scaled back; a failed matrix (info != 0) raises the no-convergence flag.
__global__ void __launch_bounds__(256) eigh_finish_kernel(double* __restrict__ U, double* __restrict__ E, int n,
                                                          const double* __restrict__ scale, const int* __restrict__ info,
                                                          int* __restrict__ flag) {
    const int64_t mat = blockIdx.y;
    double* B = U + (size_t)mat * n * n * 2;
    const double sc = scale[mat];
    const bool nan_out = sc != sc;
    const double qnan = __builtin_nan("");
    const size_t count = (size_t)n * n;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < count; e += (size_t)gridDim.x * 256) {
        const size_t r = e / n, c = e % n;
        if (c < r) continue;
        const size_t t = c * n + r;
        const double ur = B[2 * e], ui = B[2 * e + 1], vr = B[2 * t], vi = B[2 * t + 1];
        B[2 * e] = nan_out ? qnan : vr;
        B[2 * e + 1] = nan_out ? qnan : -vi;
        B[2 * t] = nan_out ? qnan : ur;
        B[2 * t + 1] = nan_out ? qnan : -ui;
    }
    if (blockIdx.x == 0) {
        for (int j = threadIdx.x; j < n; j += 256) E[(size_t)mat * n + j] = nan_out ? qnan : E[(size_t)mat * n + j] * sc;
        if (threadIdx.x == 0) {
            if (nan_out) atomicAdd(flag + 1, 1);
            else if (info[mat] != 0) atomicAdd(flag, 1);
        }
    }
}

int eigh_rocsolver(tbk_model* m, double* d_U, int64_t nk, double* d_E) {
    const int n = m->n_orb;
    TBK_CHECK(m->ws_E.reserve((size_t)nk * n * sizeof(double)));
    TBK_CHECK(m->ws_info.reserve((size_t)nk * sizeof(int)));
    TBK_CHECK(m->ws_E2.reserve((size_t)nk * sizeof(double)));
    StageTimer t(m, TBK_T_EIG);
    hipLaunchKernelGGL(eigh_scale_kernel, dim3((unsigned)nk), dim3(256), 0, m->stream, d_U, n, m->ws_E2.as<double>());
    TBK_HIP(hipGetLastError());
    TBK_ROCBLAS(rocsolver_zheev_strided_batched(
        m->blas, rocblas_evect_original, rocblas_fill_lower, n, reinterpret_cast<rocblas_double_complex*>(d_U), n,
        (rocblas_stride)n * n, d_E, (rocblas_stride)n, m->ws_E.as<double>(), (rocblas_stride)n, m->ws_info.as<int>(),
        (rocblas_int)nk));
    const unsigned gx = (unsigned)std::min<int64_t>(64, ((int64_t)n * n + 255) / 256);
    hipLaunchKernelGGL(eigh_finish_kernel, dim3(gx, (unsigned)nk), dim3(256), 0, m->stream, d_U, d_E, n,
                       m->ws_E2.as<double>(), m->ws_info.as<int>(), m->ws_flag.as<int>());
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

int eigh_jacobi(tbk_model* m, double* d_U, int64_t nk, double* d_E) {
    StageTimer t(m, TBK_T_EIG);
    const int n = m->n_orb;
    if (n <= 8) return launch_jacobi<8>(m, d_U, nk, d_E);
    if (n <= 16) return launch_jacobi<16>(m, d_U, nk, d_E);
    if (n <= 32) return launch_jacobi<32>(m, d_U, nk, d_E);
    return launch_jacobi<64>(m, d_U, nk, d_E);
}

}  // namespace

// What needs no model is checked before the model is touched (tbk_eigh_multi and the k.p entries too).
int tbk_eigh_check_arguments(int64_t nk, int convention, const double* pos) {
    TBK_ARG(convention == 1 || convention == 2, "convention must be 1 or 2");
    TBK_ARG(convention == 2 || pos != nullptr, "convention 1 needs pos");
    TBK_ARG(nk >= 0, "nk < 0");
    return TBK_OK;
}

// tbk_eigh_device; caller_rows: H(k) of every chunk from finished phase rows on the classical paths (tbk_hk_plan), so that a k-point's
// bits do not depend on the chunk being one point long (which otherwise takes the one-launch kernel)
int tbk_eigh_device_rows(tbk_model* m, const double* d_k, int64_t nk, int convention, const double* d_pos, double* d_E, double* d_U,
                         bool caller_rows) {
    TBK_CHECK(tbk_eigh_check_arguments(nk, convention, d_pos));
    TBK_ARG(m != nullptr, "model is NULL");
    TBK_LOCK(m);
    if (nk == 0 || m->n_orb == 0) return TBK_OK;
    TBK_ARG(d_k && d_E && d_U, "k / E / U is NULL");
    TBK_CHECK(tbk_eig_check_option(m));
    TBK_HIP(hipSetDevice(m->device));
    // eigenvectors: the Jacobi kernel where eigenval takes the register-resident family, rocSOLVER everywhere else
    const bool own = tbk_eig_plan(m->n_orb, m->eigensolver, nk).family == EIG_REGISTER;
    int64_t chunk = choose_chunk(m, nk, true);
    const size_t n = (size_t)m->n_orb, nn2 = n * n * 2;
    if (!own) {
        // (tbk_api.hip eigenval_device_impl: rocsolver_zheevd_strided_batched calls stay below 2^29 elements)
        chunk = std::max<int64_t>(1, std::min<int64_t>(chunk, (int64_t(1) << 29) / (int64_t)(n * n)));
        m->counters[TBK_CNT_LIBRARY_CALLS] += 1;
    }
    for (int64_t c0 = 0; c0 < nk; c0 += chunk) {
        const int64_t nkc = std::min(chunk, nk - c0);
        const tbk_hk_plan_t plan = tbk_hk_plan(m, tbk_staged_operand(m), nkc, caller_rows, caller_rows);
        double* Uc = d_U + (size_t)c0 * nn2;
        double* Ec = d_E + (size_t)c0 * n;
        TBK_CHECK(chunk_h(m, plan, HK_FULL, convention, d_k + c0 * m->dim, d_pos, tbk_one_k_t(), Uc));
        TBK_CHECK(own ? eigh_jacobi(m, Uc, nkc, Ec) : eigh_rocsolver(m, Uc, nkc, Ec));
    }
    return TBK_OK;
}

extern "C" int tbk_eigh_device(tbk_model* m, const double* d_k, int64_t nk, int convention, const double* d_pos, double* d_E,
                               double* d_U) {
    return tbk_eigh_device_rows(m, d_k, nk, convention, d_pos, d_E, d_U, false);
}

// Host buffers: k (and pos) go up through the pinned staging buffer when they fit, E and U come down in pieces of at most
// 128 MiB of U (one device buffer each), and the flags are checked once at the end (tbk_eigenval_check: synchronises).
extern "C" int tbk_eigh(tbk_model* m, const double* k, int64_t nk, int convention, const double* pos, double* E_out,
                        double* U_out) {
    TBK_CHECK(tbk_eigh_check_arguments(nk, convention, pos));
    TBK_ARG(m != nullptr, "model is NULL");
    TBK_LOCK(m);
    if (nk == 0 || m->n_orb == 0) return TBK_OK;
    TBK_ARG(k && E_out && U_out, "k / E / U is NULL");
    TBK_HIP(hipSetDevice(m->device));
    const size_t n = (size_t)m->n_orb, nn2 = n * n * 2;
    const size_t k_bytes = (size_t)nk * m->dim * sizeof(double);
    const size_t p_bytes = convention == 1 ? n * m->dim * sizeof(double) : 0;
    TBK_CHECK(m->ws_k.reserve(k_bytes));
    const double* d_pos = nullptr;
    if (convention == 1) {
        TBK_CHECK(m->ws_pos.reserve(p_bytes));
        d_pos = m->ws_pos.as<double>();
    }
    const bool staged_in = m->h_stage != nullptr && k_bytes + p_bytes <= m->h_stage_bytes;
    if (staged_in) {
        char* st = static_cast<char*>(m->h_stage.h);
        std::memcpy(st, k, k_bytes);
        if (p_bytes) std::memcpy(st + k_bytes, pos, p_bytes);
        TBK_HIP(hipMemcpyAsync(m->ws_k.ptr, st, k_bytes, hipMemcpyHostToDevice, m->stream));
        if (p_bytes) TBK_HIP(hipMemcpyAsync(m->ws_pos.ptr, st + k_bytes, p_bytes, hipMemcpyHostToDevice, m->stream));
    } else {
        TBK_HIP(hipMemcpyAsync(m->ws_k.ptr, k, k_bytes, hipMemcpyHostToDevice, m->stream));
        if (p_bytes) TBK_HIP(hipMemcpyAsync(m->ws_pos.ptr, pos, p_bytes, hipMemcpyHostToDevice, m->stream));
    }
    const int64_t piece = std::max<int64_t>(1, std::min<int64_t>(nk, (int64_t)((size_t(128) << 20) / (nn2 * sizeof(double)))));
    TBK_CHECK(m->ws_out.reserve((size_t)piece * nn2 * sizeof(double)));
    TBK_CHECK(m->ws_out2.reserve((size_t)piece * n * sizeof(double)));
    for (int64_t c0 = 0; c0 < nk; c0 += piece) {
        const int64_t nkc = std::min(piece, nk - c0);
        const size_t u_bytes = (size_t)nkc * nn2 * sizeof(double), e_bytes = (size_t)nkc * n * sizeof(double);
        TBK_CHECK(tbk_eigh_device(m, m->ws_k.as<double>() + c0 * m->dim, nkc, convention, d_pos, m->ws_out2.as<double>(),
                                  m->ws_out.as<double>()));
        // (a small result comes down through the pinned buffer -- after the upload has left it: same stream)
        if (staged_in && nkc == nk && u_bytes + e_bytes <= m->h_stage_bytes) {
            char* st = static_cast<char*>(m->h_stage.h);
            TBK_HIP(hipMemcpyAsync(st, m->ws_out.ptr, u_bytes, hipMemcpyDeviceToHost, m->stream));
            TBK_HIP(hipMemcpyAsync(st + u_bytes, m->ws_out2.ptr, e_bytes, hipMemcpyDeviceToHost, m->stream));
            TBK_CHECK(tbk_eigenval_check(m));  // synchronises
            std::memcpy(U_out, st, u_bytes);
            std::memcpy(E_out, st + u_bytes, e_bytes);
            return TBK_OK;
        }
        TBK_HIP(hipMemcpyAsync(U_out + (size_t)c0 * nn2, m->ws_out.ptr, u_bytes, hipMemcpyDeviceToHost, m->stream));
        TBK_HIP(hipMemcpyAsync(E_out + (size_t)c0 * n, m->ws_out2.ptr, e_bytes, hipMemcpyDeviceToHost, m->stream));
    }
    return tbk_eigenval_check(m);  // synchronises
}

extern "C" int tbk_kdotp_eigh(tbk_kdotp* kp, const double* k, int64_t nk, double* E_out, double* U_out) {
    TBK_CHECK(tbk_eigh_check_arguments(nk, 2, nullptr));
    TBK_ARG(kp != nullptr, "model is NULL");
    return tbk_eigh(kp->core, k, nk, 2, nullptr, E_out, U_out);
}
