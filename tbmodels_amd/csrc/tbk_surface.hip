// tbk_surface.hip -- surface and bulk Green's functions of a semi-infinite crystal by the iterative decimation of Lopez Sancho, Lopez
// Sancho and Rubio (J. Phys. F 15, 851 (1985)).  Not in the reference; DESIGN.md section 21 has the quantity, the kernels and the
// measurements, tools/surface_model.py is the statement the tests compare with.
//
//   H_m(kp)  = sum_{R : R_a = m} exp(2 pi i kp.Rp) hop_full[R]        a: the stacking axis, m = -L ... L, L = max |R_a|
//   H00[p,q] = H_{q-p},  H01[p,q] = H_{L+q-p} (q <= p), else 0        principal layers of L cells: N = n L (n when L = 0)
//
//   es = et = e = H00, alpha = H01, beta = H01^H;  repeat
//       g = (z 1 - e)^-1
//       T = g alpha:  A' = alpha T,  et += beta T,  e += beta T
//       T = g beta:   es += alpha T, e += alpha T,  B' = beta T
//       alpha, beta = A', B'
//   until max(|alpha|_inf, |beta|_inf) <= 2^-53 |H01|_inf  (row sums of |re| + |im|);
//   G_bottom = (z - es)^-1, G_top = (z - et)^-1, G_bulk = (z - e)^-1.
//
//   surface_layers_kernel    H00, H01 of a chunk's in-plane points from the FULL H(k) at k_a = j / (2 L + 1), j = 0 ... 2 L (chunk_h,
//                            convention 2): H_m = (1 / (2 L + 1)) sum_j exp(-2 pi i m j / (2 L + 1)) H(kp, j / (2 L + 1)), the twiddles
//                            from a host table.  No line of the H(k) path knows about surfaces.
//   surface_decimate_kernel  one workgroup owns one (kp, z) for the whole iteration: the inversion is green_invert_kernel's panelled
//                            Gauss-Jordan (zgj_invert of tbk_zmfma.h on the X planes), the six products per iteration run on
//                            v_mfma_f64_16x16x4_f64, four real MFMAs per complex tile and K step.  N <= 64.
//   surf_lib_chunk           65 <= N <= 1024, and on request: the same iteration in lockstep batches of a fixed number of members on
//                            rocblas_zgemm_strided_batched and rocsolver_zgetrf / zgetri_strided_batched, with five small kernels.
//
// And the Landauer transmission through a device of M principal layers between two leads of the crystal (DESIGN.md section 22,
// tools/transport_model.py): es and et of the decimation are H00 plus the leads' self-energies, a recursive sweep over the layers
// gives P_M = G_{M,1}, and T = Re tr[(Gamma_R P_M) (Gamma_L P_M^H)].
//
//   transmission_kernel      one workgroup owns one (kp, z) from the first decimation step (surf_load, surf_iterate: the loop of
//                            surface_decimate_kernel) through one inversion and four products per layer to the trace.  N <= 64.
//   trans_lib_chunk          65 <= N <= 1024, and on request: the lead part is surf_lib_iterate, the sweep M lockstep rounds.
//   trans_ens_lib_chunk      the same route for the ensemble of tbk_ensemble.hip: surf_lib_iterate once per
//                            batch, the sweep (trans_lib_sweep, shared with trans_lib_chunk) once per sample.

#include "tbk_layered.h"

namespace {

// H00, H01: [n_k][n][n] of the chunk's in-plane points (H01 NULL: no hopping between layers, no iteration); z: [n_z].  Item w = k n_z +
// energy index; a workgroup takes the items blockIdx.x, blockIdx.x + gridDim.x, ...  Results per item: iterations, and bottom / top /
// bulk as [n][n] complex or, spectral, [n] doubles -Im diag / pi.  key0: (index of the chunk's first point) * SURF_MAX_Z; the status
// word takes the smallest ((point index * SURF_MAX_Z + energy index) * 2 + reason), reason 0 singular, 1 no convergence.  ws: the
// workgroups' slots at NP = 64.  No index depends on a value but through the pivot tables, which are permutations of [0, n).
template <int NP>
__global__ void __launch_bounds__(SurfGeom<NP>::THREADS)
    surface_decimate_kernel(const double2* __restrict__ H00, const double2* __restrict__ H01, const double2* __restrict__ z, int n_z, int n, int64_t items,
                            int max_it, int spectral, unsigned long long key0, double* ws, int32_t* __restrict__ iters, double* __restrict__ out_b,
                            double* __restrict__ out_t, double* __restrict__ out_m, unsigned long long* __restrict__ flag) {
    using Geo = SurfGeom<NP>;
    constexpr int THREADS = Geo::THREADS, S = Geo::S, SM = Geo::SM;
    extern __shared__ double surf_lds[];
    const int tid = (int)threadIdx.x;
    const SurfPlanes P = surf_planes<NP, 5>(surf_lds, ws);
    double *xr = P.xr, *xi = P.xi, *er = P.er, *ei = P.ei, *esr = P.esr, *esi = P.esi, *etr = P.etr, *eti = P.eti;
    int *prow = P.prow, *jrow = P.jrow;

    for (int64_t w = blockIdx.x; w < items; w += gridDim.x) {
        const int64_t k = w / n_z;
        const int zi = (int)(w - k * n_z);
        const double2 zz = z[zi];
        const double2* h0 = H00 + (size_t)k * n * n;
        const bool hops = H01 != nullptr;
        const double2* h1 = hops ? H01 + (size_t)k * n * n : H00;
        surf_load<NP>(P, h0, h1, hops, n, tid);
        int it = 0, status = 0;  // status 1: singular, 2: the cap was reached (the same on every thread)
        if (hops) status = surf_iterate<NP>(P, zz, n, max_it, tid, it);
        bool bad = status == 1;
#pragma unroll 1
        for (int which = 0; which < 3; ++which) {
            const double* mr = which == 0 ? esr : which == 1 ? etr : er;
            const double* mi = which == 0 ? esi : which == 1 ? eti : ei;
            double* out = which == 0 ? out_b : which == 1 ? out_t : out_m;
            surf_form<NP, THREADS, SM>(xr, xi, mr, mi, zz, n, tid, jrow);
            bad |= zgj_invert<NP, THREADS>(xr, xi, prow, jrow, n, tid);
            __syncthreads();
            // (every element of the inverse is looked at in both modes: the same inputs are singular with and without spectral)
            double2* o = reinterpret_cast<double2*>(out) + (size_t)w * n * n;
            for (int e = tid; e < n * n; e += THREADS) {
                const int r = e / n, s = e - r * n;
                const int at = prow[r] * S + jrow[s];
                const double2 v = make_double2(xr[at], xi[at]);
                bad |= !(fabs(v.x) <= DBL_MAX && fabs(v.y) <= DBL_MAX);
                if (!spectral)
                    o[e] = v;
                else if (r == s)
                    out[(size_t)w * n + r] = -v.y / SURF_PI;
            }
            __syncthreads();  // X and the tables are free again
        }
        if (tid == 0) iters[w] = it;
        const unsigned long long key = (key0 + (unsigned long long)k * (unsigned long long)SURF_MAX_Z + (unsigned long long)zi) * 2ull;
        if (bad) atomicMin(flag, key);
        if (status == 2 && tid == 0) atomicMin(flag, key + 1ull);
    }
}

// H00, H01, z, items, key0, ws, iters, flag: surface_decimate_kernel's (H01 is not NULL).  V: [m_layers][n][n], the same for every item.
// One workgroup owns an item from the first decimation step to the trace: T_out[item], and P_M [n][n] into G_out unless it is NULL.
// Status: a zero pivot or a non-finite element of a g_p or of P_M is reason 0, the cap of the decimation reason 1.  Every branch is
// workgroup-uniform; no index depends on a value but through the pivot tables.  The sweep itself is tbk_surface.h's.
template <int NP>
__global__ void __launch_bounds__(SurfGeom<NP>::THREADS)
    transmission_kernel(const double2* __restrict__ H00, const double2* __restrict__ H01, const double2* __restrict__ V, int m_layers,
                        const double2* __restrict__ z, int n_z, int n, int64_t items, int max_it, unsigned long long key0, double* ws,
                        int32_t* __restrict__ iters, double* __restrict__ T_out, double2* __restrict__ G_out, unsigned long long* __restrict__ flag) {
    extern __shared__ double surf_lds[];
    const int tid = (int)threadIdx.x;
    const SurfPlanes P = surf_planes<NP, TransGeom<NP>::MATS>(surf_lds, ws);

    for (int64_t w = blockIdx.x; w < items; w += gridDim.x) {
        const int64_t k = w / n_z;
        const int zi = (int)(w - k * n_z);
        const double2 zz = z[zi];
        const double2* h0 = H00 + (size_t)k * n * n;
        const double2* h1 = H01 + (size_t)k * n * n;
        surf_load<NP>(P, h0, h1, true, n, tid);
        int it = 0;
        const int status = surf_iterate<NP>(P, zz, n, max_it, tid, it);  // 1: singular, 2: the cap (the same on every thread)
        bool bad = status == 1;
        trans_start<NP>(P, h1, V, n, tid);
#pragma unroll 1
        for (int p = 0; p < m_layers; ++p) bad |= trans_layer<NP, false>(P, h0, V, zz, p, m_layers, n, tid, nullptr);
        bad |= trans_closing<NP>(P, n, tid, G_out != nullptr ? G_out + (size_t)w * n * n : nullptr, T_out + w, iters + w, it);
        const unsigned long long key = (key0 + (unsigned long long)k * (unsigned long long)SURF_MAX_Z + (unsigned long long)zi) * 2ull;
        if (bad) atomicMin(flag, key);
        if (status == 2 && tid == 0) atomicMin(flag, key + 1ull);
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
struct SurfShape {
    int n = 0;             // rows of a principal layer
    int64_t n_z = 0;
    bool spectral = false;
    size_t item_doubles() const { return spectral ? (size_t)n : (size_t)n * n * 2; }  // of one of the three results
    size_t out_bytes(int64_t nk) const { return dos_align256((size_t)nk * n_z * item_doubles() * sizeof(double)); }
    size_t it_bytes(int64_t nk) const { return dos_align256((size_t)nk * n_z * sizeof(int32_t)); }
    size_t result_bytes(int64_t nk) const { return 3 * out_bytes(nk) + it_bytes(nk); }  // bottom, top, bulk, iterations
    int64_t auto_chunk(int64_t nk) const {
        const size_t per_k = (size_t)n_z * (3 * item_doubles() * sizeof(double) + sizeof(int32_t));
        return std::max<int64_t>(1, std::min<int64_t>(nk, (int64_t)(SURF_CHUNK_BUDGET / per_k)));
    }
};

template <int NP>
int surf_launch_np(hipStream_t s, int n_cu, const SurfShape& sh, const double2* d_H00, const double2* d_H01, const double2* d_z, int64_t nkc, int max_it,
                   unsigned long long key0, double* d_ws, char* d_res) {
    using Geo = SurfGeom<NP>;
    static tbk_flag_row done;  // of this instantiation's kernel
    const int64_t items = nkc * sh.n_z;
    if (Geo::lds_bytes > SURF_LDS_DEFAULT)
        TBK_HIP(tbk_raise_lds_limit(reinterpret_cast<const void*>(surface_decimate_kernel<NP>), (int)Geo::lds_bytes, done));
    double* d_b = reinterpret_cast<double*>(d_res);
    double* d_t = reinterpret_cast<double*>(d_res + sh.out_bytes(nkc));
    double* d_m = reinterpret_cast<double*>(d_res + 2 * sh.out_bytes(nkc));
    int32_t* d_it = reinterpret_cast<int32_t*>(d_res + 3 * sh.out_bytes(nkc));
    hipLaunchKernelGGL(surface_decimate_kernel<NP>, dim3((unsigned)surf_grid(sh.n, items, n_cu)), dim3(Geo::THREADS), Geo::lds_bytes, s, d_H00, d_H01,
                       d_z, (int)sh.n_z, sh.n, items, max_it, sh.spectral ? 1 : 0, key0, d_ws, d_it, d_b, d_t, d_m,
                       reinterpret_cast<unsigned long long*>(d_res + sh.result_bytes(nkc)));
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

// The decimation of the chunk's nkc points at every energy.  d_res: bottom, top, bulk, iterations of the chunk (SurfShape's
// offsets for nkc points) and, behind them, the status word.
int surf_launch(hipStream_t s, int n_cu, const SurfShape& sh, const double2* d_H00, const double2* d_H01, const double2* d_z, int64_t nkc, int max_it,
                int64_t k0, double* d_ws, char* d_res) {
    const unsigned long long key0 = (unsigned long long)k0 * (unsigned long long)SURF_MAX_Z;
    return surf_with_np(sh.n, [&](auto np) { return surf_launch_np<decltype(np)::value>(s, n_cu, sh, d_H00, d_H01, d_z, nkc, max_it, key0, d_ws, d_res); });
}

// ---- above 64 rows, and on request: the library route ---------------------------------------------------------------------------------
// The (k, z) of a chunk in lockstep, in batches of a FIXED number of members (a function of N alone; the last batch is filled with
// dummy members, zero matrices): rocblas_zgemm_strided_batched for the six products, rocsolver_zgetrf / zgetri_strided_batched for the
// inversions, small kernels for z - e, the sums, the norms and the results.  The batch count never changes, so the library is asked the
// same question whatever the chunk and the list; a member that has converged gets alpha = beta = 0 exactly and later iterations add
// exact zeros to it.  Matrices are row-major: the library reads them as their transposes, so C = A B is the library's product of B
// and A, and the in-place inverse of a transpose is the transpose of the inverse (20.2).
constexpr size_t SURF_LIB_BUDGET = size_t(512) << 20;
constexpr int SURF_LIB_MATRICES = 10;  // alpha, beta, their successors, e, es, et, A (g), T, one product

int surf_lib_batch(int n) {
    const size_t per = (size_t)SURF_LIB_MATRICES * n * n * sizeof(double2);
    return (int)std::max<size_t>(1, std::min<size_t>(64, SURF_LIB_BUDGET / per));
}

struct SurfLib {
    rocblas_handle blas = nullptr;
    int n = 0, batch = 0;
    double2* mat[SURF_LIB_MATRICES] = {};
    int* ipiv = nullptr;    // [batch][n]
    int* info = nullptr;    // [2][batch] of getrf and getri
    int* done = nullptr;    // [batch]
    int* active = nullptr;  // one word: members still iterating
    double* thr = nullptr;  // [batch]
    static size_t bytes(int n, int batch) {
        return (size_t)SURF_LIB_MATRICES * dos_align256((size_t)batch * n * n * sizeof(double2)) + dos_align256((size_t)batch * n * sizeof(int)) +
               dos_align256((size_t)(3 * batch + 1) * sizeof(int)) + dos_align256((size_t)batch * sizeof(double));
    }
    void place(char* base, int n_, int batch_, rocblas_handle h) {
        n = n_;
        batch = batch_;
        blas = h;
        const size_t mb = dos_align256((size_t)batch * n * n * sizeof(double2));
        for (int i = 0; i < SURF_LIB_MATRICES; ++i) mat[i] = reinterpret_cast<double2*>(base + (size_t)i * mb);
        char* at = base + (size_t)SURF_LIB_MATRICES * mb;
        ipiv = reinterpret_cast<int*>(at);
        at += dos_align256((size_t)batch * n * sizeof(int));
        info = reinterpret_cast<int*>(at);
        done = info + 2 * batch;
        active = done + batch;
        at += dos_align256((size_t)(3 * batch + 1) * sizeof(int));
        thr = reinterpret_cast<double*>(at);
    }
};

// member b of the batch is item w0 + b of the chunk (k = item / n_z), a dummy beyond `items`
__global__ void __launch_bounds__(256) surf_lib_load_kernel(const double2* __restrict__ H00, const double2* __restrict__ H01, int n_z, int n, int64_t w0,
                                                            int64_t items, double2* __restrict__ al, double2* __restrict__ be, double2* __restrict__ e,
                                                            double2* __restrict__ es, double2* __restrict__ et, int32_t* __restrict__ iters) {
    const int b = (int)blockIdx.x;
    const int64_t w = w0 + b;
    const bool valid = w < items;
    const size_t nn = (size_t)n * n, k = valid ? (size_t)(w / n_z) : 0;
    for (size_t x = (size_t)blockIdx.y * 256 + threadIdx.x; x < nn; x += (size_t)gridDim.y * 256) {
        const size_t i = x / n, c = x - i * n;
        double2 a = make_double2(0.0, 0.0), h = make_double2(0.0, 0.0);
        if (valid) {
            a = H00[k * nn + x];
            if (H01 != nullptr) h = H01[k * nn + x];
        }
        e[b * nn + x] = es[b * nn + x] = et[b * nn + x] = a;
        al[b * nn + x] = h;
        be[b * nn + c * n + i] = make_double2(h.x, -h.y);
    }
    if (valid && blockIdx.y == 0 && threadIdx.x == 0) iters[w] = 0;
}

__global__ void __launch_bounds__(256) surf_lib_form_kernel(const double2* __restrict__ M, const double2* __restrict__ z, int n_z, int n, int64_t w0,
                                                            double2* __restrict__ A) {
    const int b = (int)blockIdx.x;
    const double2 zz = z[(w0 + b) % n_z];  // (a dummy member takes some energy of the list: z 1 is invertible)
    const size_t nn = (size_t)n * n;
    for (size_t x = (size_t)blockIdx.y * 256 + threadIdx.x; x < nn; x += (size_t)gridDim.y * 256) {
        const size_t i = x / n, c = x - i * n;
        const double2 m = M[b * nn + x];
        A[b * nn + x] = make_double2((i == c ? zz.x : 0.0) - m.x, (i == c ? zz.y : 0.0) - m.y);
    }
}

__global__ void __launch_bounds__(256) surf_lib_add_kernel(const double2* __restrict__ src, size_t count, double2* __restrict__ d1, double2* __restrict__ d2) {
    for (size_t x = (size_t)blockIdx.x * 256 + threadIdx.x; x < count; x += (size_t)gridDim.x * 256) {
        const double2 v = src[x];
        double2 a = d1[x], b = d2[x];
        a.x += v.x;
        a.y += v.y;
        b.x += v.x;
        b.y += v.y;
        d1[x] = a;
        d2[x] = b;
    }
}

// One workgroup per member: |alpha|_inf, |beta|_inf (row sums of |re| + |im|, a thread per row, columns ascending).  it = 0: the
// threshold 2^-53 |H01|_inf, done cleared.  it > 0, member not done: a failed library call or a non-finite norm raises the word
// (singular), a norm at or below the threshold ends the member, the cap raises the word; an ended member records its count and gets
// alpha = beta = 0; the others count themselves in *active.
__global__ void __launch_bounds__(256) surf_lib_norms_kernel(double2* al, double2* be, int n, int batch, int64_t w0, int64_t items, int n_z, int it, int max_it,
                                                             unsigned long long key0, const int* __restrict__ info, int* done, double* thr, int* active,
                                                             int32_t* iters, unsigned long long* flag) {
    __shared__ double red[2][256];
    __shared__ int verdict;
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int64_t w = w0 + b;
    const bool valid = w < items;
    const size_t nn = (size_t)n * n;
    double2* a = al + b * nn;
    double2* bb = be + b * nn;
    if (it > 0 && done[b] != 0) return;  // (the same for every thread)
    double ma = 0.0, mb = 0.0;
    for (int r = tid; r < n; r += 256) {
        double sa = 0.0, sb = 0.0;
        for (int c = 0; c < n; ++c) {
            const double2 x = a[(size_t)r * n + c], y = bb[(size_t)r * n + c];
            sa += fabs(x.x) + fabs(x.y);
            sb += fabs(y.x) + fabs(y.y);
        }
        if (!(sa <= DBL_MAX)) sa = __builtin_inf();
        if (!(sb <= DBL_MAX)) sb = __builtin_inf();
        ma = sa > ma ? sa : ma;
        mb = sb > mb ? sb : mb;
    }
    red[0][tid] = ma;
    red[1][tid] = mb;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) {
            red[0][tid] = red[0][tid + off] > red[0][tid] ? red[0][tid + off] : red[0][tid];
            red[1][tid] = red[1][tid + off] > red[1][tid] ? red[1][tid + off] : red[1][tid];
        }
        __syncthreads();
    }
    if (tid == 0) {
        int v = 0;  // 0: goes on, 1: ended
        if (it == 0) {
            thr[b] = red[0][0] * 0x1p-53;
            done[b] = 0;
        } else {
            const double size = red[0][0] > red[1][0] ? red[0][0] : red[1][0];
            const unsigned long long key = (key0 + (unsigned long long)(w / n_z) * (unsigned long long)SURF_MAX_Z + (unsigned long long)(w % n_z)) * 2ull;
            if (info[b] != 0 || info[batch + b] != 0 || !(size <= DBL_MAX)) {
                v = 1;
                if (valid) atomicMin(flag, key);
            } else if (size <= thr[b]) {
                v = 1;
            } else if (it >= max_it) {
                v = 1;
                if (valid) atomicMin(flag, key + 1ull);
            } else {
                atomicAdd(active, 1);
            }
            if (v == 1) {
                done[b] = 1;
                if (valid) iters[w] = it;
            }
        }
        verdict = v;
    }
    __syncthreads();
    if (verdict == 1)
        for (size_t x = tid; x < nn; x += 256) a[x] = bb[x] = make_double2(0.0, 0.0);
}

// the closing inverses of the batch into the chunk's results
__global__ void __launch_bounds__(256) surf_lib_out_kernel(const double2* __restrict__ A, const int* __restrict__ info, int n, int batch, int64_t w0, int64_t items,
                                                           int n_z, int spectral, unsigned long long key0, double* __restrict__ out,
                                                           unsigned long long* __restrict__ flag) {
    const int b = (int)blockIdx.x;
    const int64_t w = w0 + b;
    if (w >= items) return;
    const size_t nn = (size_t)n * n;
    const double2* g = A + b * nn;
    bool bad = info[b] != 0 || info[batch + b] != 0;
    for (size_t x = (size_t)blockIdx.y * 256 + threadIdx.x; x < nn; x += (size_t)gridDim.y * 256) {
        const double2 v = g[x];
        bad |= !(fabs(v.x) <= DBL_MAX && fabs(v.y) <= DBL_MAX);
        const size_t i = x / n, c = x - i * n;
        if (spectral) {
            if (i == c) out[(size_t)w * n + i] = -v.y / SURF_PI;
        } else {
            reinterpret_cast<double2*>(out)[(size_t)w * nn + x] = v;
        }
    }
    if (bad) atomicMin(flag, (key0 + (unsigned long long)(w / n_z) * (unsigned long long)SURF_MAX_Z + (unsigned long long)(w % n_z)) * 2ull);
}

// row-major C = A B for every member
int surf_lib_gemm(const SurfLib& W, const double2* A, const double2* B, double2* C) {
    const rocblas_double_complex one(1.0, 0.0), zero(0.0, 0.0);
    const rocblas_stride st = (rocblas_stride)W.n * W.n;
    TBK_ROCBLAS(rocblas_zgemm_strided_batched(W.blas, rocblas_operation_none, rocblas_operation_none, W.n, W.n, W.n, &one,
                                              reinterpret_cast<const rocblas_double_complex*>(B), W.n, st,
                                              reinterpret_cast<const rocblas_double_complex*>(A), W.n, st, &zero,
                                              reinterpret_cast<rocblas_double_complex*>(C), W.n, st, W.batch));
    return TBK_OK;
}

// A = (z 1 - M)^-1 for every member, in place; the two status rows in W.info
int surf_lib_invert(hipStream_t s, const SurfLib& W, const double2* M, const double2* d_z, int n_z, int64_t w0, double2* A) {
    const unsigned gy = (unsigned)std::min<size_t>(64, ((size_t)W.n * W.n + 255) / 256);
    hipLaunchKernelGGL(surf_lib_form_kernel, dim3((unsigned)W.batch, gy), dim3(256), 0, s, M, d_z, n_z, W.n, w0, A);
    TBK_HIP(hipGetLastError());
    rocblas_double_complex* a = reinterpret_cast<rocblas_double_complex*>(A);
    const rocblas_stride st = (rocblas_stride)W.n * W.n;
    TBK_ROCBLAS(rocsolver_zgetrf_strided_batched(W.blas, W.n, W.n, a, W.n, st, W.ipiv, (rocblas_stride)W.n, W.info, W.batch));
    TBK_ROCBLAS(rocsolver_zgetri_strided_batched(W.blas, W.n, a, W.n, st, W.ipiv, (rocblas_stride)W.n, W.info + W.batch, W.batch));
    return TBK_OK;
}

// The iteration of the batch that starts at item w0: afterwards es and et are in W.mat[5] and W.mat[6], e in W.mat[4]; the other
// matrices are free.  The host reads one word per iteration: how many members go on.
int surf_lib_iterate(hipStream_t s, const SurfLib& W, const double2* d_H00, const double2* d_H01, const double2* d_z, int n_z, int64_t items, int64_t w0,
                     int max_it, unsigned long long key0, int32_t* d_it, unsigned long long* d_flag) {
    const int n = W.n;
    const size_t count = (size_t)W.batch * n * n;
    const unsigned gy = (unsigned)std::min<size_t>(64, ((size_t)n * n + 255) / 256);
    const unsigned ga = (unsigned)std::min<size_t>(4096, (count + 255) / 256);
    double2 *al = W.mat[0], *be = W.mat[1], *al2 = W.mat[2], *be2 = W.mat[3];
    double2 *e = W.mat[4], *es = W.mat[5], *et = W.mat[6], *A = W.mat[7], *T = W.mat[8], *V = W.mat[9];
    hipLaunchKernelGGL(surf_lib_load_kernel, dim3((unsigned)W.batch, gy), dim3(256), 0, s, d_H00, d_H01, n_z, n, w0, items, al, be, e, es, et, d_it);
    TBK_HIP(hipGetLastError());
    if (d_H01 != nullptr) {
        hipLaunchKernelGGL(surf_lib_norms_kernel, dim3((unsigned)W.batch), dim3(256), 0, s, al, be, n, W.batch, w0, items, n_z, 0, max_it, key0, W.info,
                           W.done, W.thr, W.active, d_it, d_flag);
        TBK_HIP(hipGetLastError());
        for (int it = 1; it <= max_it; ++it) {
            TBK_CHECK(surf_lib_invert(s, W, e, d_z, n_z, w0, A));
            TBK_CHECK(surf_lib_gemm(W, A, al, T));    // T = g alpha
            TBK_CHECK(surf_lib_gemm(W, al, T, al2));  // alpha g alpha
            TBK_CHECK(surf_lib_gemm(W, be, T, V));    // beta g alpha
            hipLaunchKernelGGL(surf_lib_add_kernel, dim3(ga), dim3(256), 0, s, V, count, et, e);
            TBK_CHECK(surf_lib_gemm(W, A, be, T));    // T = g beta
            TBK_CHECK(surf_lib_gemm(W, al, T, V));    // alpha g beta
            hipLaunchKernelGGL(surf_lib_add_kernel, dim3(ga), dim3(256), 0, s, V, count, es, e);
            TBK_CHECK(surf_lib_gemm(W, be, T, be2));  // beta g beta
            std::swap(al, al2);
            std::swap(be, be2);
            TBK_HIP(hipMemsetAsync(W.active, 0, sizeof(int), s));
            hipLaunchKernelGGL(surf_lib_norms_kernel, dim3((unsigned)W.batch), dim3(256), 0, s, al, be, n, W.batch, w0, items, n_z, it, max_it, key0,
                               W.info, W.done, W.thr, W.active, d_it, d_flag);
            TBK_HIP(hipGetLastError());
            int active = 0;
            TBK_HIP(hipMemcpyAsync(&active, W.active, sizeof(int), hipMemcpyDeviceToHost, s));
            TBK_HIP(hipStreamSynchronize(s));
            if (active == 0) break;
        }
    }
    return TBK_OK;
}

// The chunk's nkc points at every energy on the library route (the arguments of surf_launch).  The host reads one word per iteration
// and batch: how many members go on.
int surf_lib_chunk(hipStream_t s, const SurfLib& W, const SurfShape& sh, const double2* d_H00, const double2* d_H01, const double2* d_z, int64_t nkc,
                   int max_it, int64_t k0, char* d_res) {
    const int n = sh.n, n_z = (int)sh.n_z;
    const int64_t items = nkc * sh.n_z;
    const unsigned long long key0 = (unsigned long long)k0 * (unsigned long long)SURF_MAX_Z;
    double* outs[3] = {reinterpret_cast<double*>(d_res), reinterpret_cast<double*>(d_res + sh.out_bytes(nkc)),
                       reinterpret_cast<double*>(d_res + 2 * sh.out_bytes(nkc))};
    int32_t* d_it = reinterpret_cast<int32_t*>(d_res + 3 * sh.out_bytes(nkc));
    unsigned long long* d_flag = reinterpret_cast<unsigned long long*>(d_res + sh.result_bytes(nkc));
    const unsigned gy = (unsigned)std::min<size_t>(64, ((size_t)n * n + 255) / 256);
    for (int64_t w0 = 0; w0 < items; w0 += W.batch) {
        double2 *e = W.mat[4], *es = W.mat[5], *et = W.mat[6], *A = W.mat[7];
        TBK_CHECK(surf_lib_iterate(s, W, d_H00, d_H01, d_z, n_z, items, w0, max_it, key0, d_it, d_flag));
        const double2* closing[3] = {es, et, e};
        for (int which = 0; which < 3; ++which) {
            TBK_CHECK(surf_lib_invert(s, W, closing[which], d_z, n_z, w0, A));
            hipLaunchKernelGGL(surf_lib_out_kernel, dim3((unsigned)W.batch, gy), dim3(256), 0, s, A, W.info, n, W.batch, w0, items, n_z, sh.spectral ? 1 : 0,
                               key0, outs[which], d_flag);
            TBK_HIP(hipGetLastError());
        }
    }
    return TBK_OK;
}

// ---- the transmission: host ------------------------------------------------------------------------------------------------------------
constexpr const char* TRANS_FAMILY = "the transmission";

// The results of a chunk: T, iterations, P_M (green), and behind them the status word.
struct TransShape {
    int n = 0, m_layers = 0;
    int64_t n_z = 0;
    bool green = false;
    size_t t_bytes(int64_t nk) const { return dos_align256((size_t)nk * n_z * sizeof(double)); }
    size_t it_bytes(int64_t nk) const { return dos_align256((size_t)nk * n_z * sizeof(int32_t)); }
    size_t g_bytes(int64_t nk) const { return green ? dos_align256((size_t)nk * n_z * n * n * sizeof(double2)) : 0; }
    size_t result_bytes(int64_t nk) const { return t_bytes(nk) + it_bytes(nk) + g_bytes(nk); }
    int64_t auto_chunk(int64_t nk) const {  // the chunk's results and its two layers inside the budget
        const size_t nn = (size_t)n * n * sizeof(double2);
        const size_t per_k = (size_t)n_z * (sizeof(double) + sizeof(int32_t) + (green ? nn : 0)) + 2 * nn;
        return std::max<int64_t>(1, std::min<int64_t>(nk, (int64_t)(SURF_CHUNK_BUDGET / per_k)));
    }
};

template <int NP>
int trans_launch_np(hipStream_t s, int n_cu, const TransShape& sh, const double2* d_H00, const double2* d_H01, const double2* d_V, const double2* d_z,
                    int64_t nkc, int max_it, unsigned long long key0, double* d_ws, char* d_res) {
    using Geo = SurfGeom<NP>;
    static tbk_flag_row done;  // of this instantiation's kernel
    const int64_t items = nkc * sh.n_z;
    if (TransGeom<NP>::lds_bytes > SURF_LDS_DEFAULT)
        TBK_HIP(tbk_raise_lds_limit(reinterpret_cast<const void*>(transmission_kernel<NP>), (int)TransGeom<NP>::lds_bytes, done));
    double* d_T = reinterpret_cast<double*>(d_res);
    int32_t* d_it = reinterpret_cast<int32_t*>(d_res + sh.t_bytes(nkc));
    double2* d_G = sh.green ? reinterpret_cast<double2*>(d_res + sh.t_bytes(nkc) + sh.it_bytes(nkc)) : nullptr;
    hipLaunchKernelGGL(transmission_kernel<NP>, dim3((unsigned)surf_grid(sh.n, items, n_cu)), dim3(Geo::THREADS), TransGeom<NP>::lds_bytes, s, d_H00, d_H01,
                       d_V, sh.m_layers, d_z, (int)sh.n_z, sh.n, items, max_it, key0, d_ws, d_it, d_T, d_G,
                       reinterpret_cast<unsigned long long*>(d_res + sh.result_bytes(nkc)));
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

// The transmission of the chunk's nkc points at every energy.  d_res: TransShape's layout for nkc points.
int trans_launch(hipStream_t s, int n_cu, const TransShape& sh, const double2* d_H00, const double2* d_H01, const double2* d_V, const double2* d_z,
                 int64_t nkc, int max_it, int64_t k0, double* d_ws, char* d_res) {
    const unsigned long long key0 = (unsigned long long)k0 * (unsigned long long)SURF_MAX_Z;
    return surf_with_np(sh.n, [&](auto np) { return trans_launch_np<decltype(np)::value>(s, n_cu, sh, d_H00, d_H01, d_V, d_z, nkc, max_it, key0, d_ws, d_res); });
}

// ---- the library route of the transmission: the lead part is surf_lib_iterate, the sweep M lockstep rounds without convergence logic --
// member b of the batch: H01 and H01^H again, D_1 = et + V_1 (a dummy member: zeros, so that z 1 - D is z 1).  V: either form of trans_v
template <typename VT>
__global__ void __launch_bounds__(256) trans_lib_start_kernel(const double2* __restrict__ H01, const VT* __restrict__ V, const double2* __restrict__ et,
                                                             int n_z, int n, int64_t w0, int64_t items, double2* __restrict__ h01,
                                                             double2* __restrict__ h10, double2* __restrict__ D) {
    const int b = (int)blockIdx.x;
    const int64_t w = w0 + b;
    const bool valid = w < items;
    const size_t nn = (size_t)n * n, k = valid ? (size_t)(w / n_z) : 0;
    for (size_t x = (size_t)blockIdx.y * 256 + threadIdx.x; x < nn; x += (size_t)gridDim.y * 256) {
        const size_t i = x / n, c = x - i * n;
        double2 h = make_double2(0.0, 0.0), d = make_double2(0.0, 0.0);
        if (valid) {
            h = H01[k * nn + x];
            const double2 e = et[b * nn + x], v = trans_v(V, (int)i, (int)c, n);
            d = make_double2(e.x + v.x, e.y + v.y);
        }
        h01[b * nn + x] = h;
        h10[b * nn + c * n + i] = make_double2(h.x, -h.y);
        D[b * nn + x] = d;
    }
}

// V NULL: D += es - H00 (the right lead, `other` is es); else D = (H00 + V) + other (`other` is H01^H g H01)
template <typename VT>
__global__ void __launch_bounds__(256) trans_lib_onsite_kernel(const double2* __restrict__ H00, const VT* __restrict__ V, const double2* __restrict__ other,
                                                              int n_z, int n, int64_t w0, int64_t items, double2* __restrict__ D) {
    const int b = (int)blockIdx.x;
    const int64_t w = w0 + b;
    if (w >= items) return;  // (a dummy member keeps D = 0)
    const size_t nn = (size_t)n * n, k = (size_t)(w / n_z);
    for (size_t x = (size_t)blockIdx.y * 256 + threadIdx.x; x < nn; x += (size_t)gridDim.y * 256) {
        const double2 a = H00[k * nn + x], o = other[b * nn + x];
        double2 d;
        if (V == nullptr) {
            d = D[b * nn + x];
            d.x += o.x - a.x;
            d.y += o.y - a.y;
        } else {
            const size_t i = x / n, c = x - i * n;
            const double2 v = trans_v(V, (int)i, (int)c, n);
            d = make_double2((a.x + v.x) + o.x, (a.y + v.y) + o.y);
        }
        D[b * nn + x] = d;
    }
}

// a failed library call (info not NULL) or a non-finite element of the member's matrix raises the word (singular).  The key of the
// member is (key0 + point * SURF_MAX_Z + energy) * sub_n + sub: sub_n = 1, sub = 0 for the one device of the transmission, the
// ensemble's SURF_MAX_Z and its sample
__global__ void __launch_bounds__(256) trans_lib_check_kernel(const double2* __restrict__ A, const int* __restrict__ info, int n, int batch, int64_t w0,
                                                             int64_t items, int n_z, unsigned long long key0, unsigned long long sub_n,
                                                             unsigned long long sub, unsigned long long* __restrict__ flag) {
    const int b = (int)blockIdx.x;
    const int64_t w = w0 + b;
    if (w >= items) return;
    const size_t nn = (size_t)n * n;
    bool bad = info != nullptr && (info[b] != 0 || info[batch + b] != 0);
    for (size_t x = (size_t)blockIdx.y * 256 + threadIdx.x; x < nn; x += (size_t)gridDim.y * 256) {
        const double2 v = A[b * nn + x];
        bad |= !(fabs(v.x) <= DBL_MAX && fabs(v.y) <= DBL_MAX);
    }
    if (bad)
        atomicMin(flag, ((key0 + (unsigned long long)(w / n_z) * (unsigned long long)SURF_MAX_Z + (unsigned long long)(w % n_z)) * sub_n + sub) * 2ull);
}

// gamma = i (e - e^H) and, P not NULL, adj = P^H, for every member
__global__ void __launch_bounds__(256) trans_lib_gamma_kernel(const double2* __restrict__ e, int n, double2* __restrict__ gamma, const double2* __restrict__ P,
                                                             double2* __restrict__ adj) {
    const int b = (int)blockIdx.x;
    const size_t nn = (size_t)n * n;
    for (size_t x = (size_t)blockIdx.y * 256 + threadIdx.x; x < nn; x += (size_t)gridDim.y * 256) {
        const size_t i = x / n, c = x - i * n;
        const double2 u = e[b * nn + x], v = e[b * nn + c * n + i];
        gamma[b * nn + x] = make_double2(-(u.y + v.y), u.x - v.x);
        if (P != nullptr) {
            const double2 q = P[b * nn + c * n + i];
            adj[b * nn + x] = make_double2(q.x, -q.y);
        }
    }
}

// One workgroup per member: T = Re sum_ij A[i][j] B[j][i] in a fixed order (a thread per row, columns ascending; thread 0 adds the
// rows in order) into T_out[item * t_stride + t_at], and P_M into G_out unless it is NULL.
__global__ void __launch_bounds__(256) trans_lib_trace_kernel(const double2* __restrict__ A, const double2* __restrict__ B, const double2* __restrict__ P, int n,
                                                             int64_t w0, int64_t items, int64_t t_stride, int64_t t_at, double* __restrict__ T_out,
                                                             double2* __restrict__ G_out) {
    __shared__ double rows[SURF_LIB_MAX];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int64_t w = w0 + b;
    if (w >= items) return;  // (the same for every thread)
    const size_t nn = (size_t)n * n;
    for (int r = tid; r < n; r += 256) {
        double sum = 0.0;
        for (int c = 0; c < n; ++c) {
            const double2 x = A[b * nn + (size_t)r * n + c], y = B[b * nn + (size_t)c * n + r];
            sum += x.x * y.x - x.y * y.y;
        }
        rows[r] = sum;
    }
    __syncthreads();
    if (tid == 0) {
        double total = 0.0;
        for (int r = 0; r < n; ++r) total += rows[r];
        T_out[w * t_stride + t_at] = total;
    }
    if (G_out != nullptr)
        for (size_t x = tid; x < nn; x += 256) G_out[(size_t)w * nn + x] = P[b * nn + x];
}

// The sweep and the closing of the batch that starts at item w0, on what surf_lib_iterate left: es and et (W.mat[5], W.mat[6]) are read
// and stay, every other matrix of W is overwritten.  d_V: the device in either form of trans_v; the keys are trans_lib_check_kernel's;
// T goes to d_T[item * t_stride + t_at].
template <typename VT>
int trans_lib_sweep(hipStream_t s, const SurfLib& W, int m_layers, const double2* d_H00, const double2* d_H01, const VT* d_V, const double2* d_z, int n_z,
                    int64_t items, int64_t w0, unsigned long long key0, unsigned long long sub_n, unsigned long long sub, int64_t t_stride, int64_t t_at,
                    double* d_T, double2* d_G, unsigned long long* d_flag) {
    const int n = W.n;
    const size_t nn = (size_t)n * n, count = (size_t)W.batch * nn;
    const dim3 grid((unsigned)W.batch, (unsigned)std::min<size_t>(64, (nn + 255) / 256));
    double2 *h01 = W.mat[0], *h10 = W.mat[1], *P = W.mat[2], *Q = W.mat[3], *D = W.mat[4], *es = W.mat[5], *et = W.mat[6], *A = W.mat[7], *T = W.mat[8],
            *R = W.mat[9];
    hipLaunchKernelGGL(trans_lib_start_kernel<VT>, grid, dim3(256), 0, s, d_H01, d_V, et, n_z, n, w0, items, h01, h10, D);
    TBK_HIP(hipGetLastError());
    for (int p = 0; p < m_layers; ++p) {
        if (p == m_layers - 1)
            hipLaunchKernelGGL(trans_lib_onsite_kernel<VT>, grid, dim3(256), 0, s, d_H00, static_cast<const VT*>(nullptr), es, n_z, n, w0, items, D);
        TBK_CHECK(surf_lib_invert(s, W, D, d_z, n_z, w0, A));  // g_p
        hipLaunchKernelGGL(trans_lib_check_kernel, grid, dim3(256), 0, s, A, W.info, n, W.batch, w0, items, n_z, key0, sub_n, sub, d_flag);
        TBK_HIP(hipGetLastError());
        if (p == 0) {
            TBK_HIP(hipMemcpyAsync(P, A, count * sizeof(double2), hipMemcpyDeviceToDevice, s));  // P_1 = g_1
        } else {
            TBK_CHECK(surf_lib_gemm(W, h10, P, T));  // T = H01^H P_{p-1}
            TBK_CHECK(surf_lib_gemm(W, A, T, Q));    // P_p = g_p T
            std::swap(P, Q);
        }
        if (p + 1 < m_layers) {
            TBK_CHECK(surf_lib_gemm(W, A, h01, T));  // T = g_p H01
            TBK_CHECK(surf_lib_gemm(W, h10, T, R));  // H01^H g_p H01
            hipLaunchKernelGGL(trans_lib_onsite_kernel<VT>, grid, dim3(256), 0, s, d_H00, d_V + (size_t)(p + 1) * trans_v_layer(d_V, n), R, n_z, n, w0, items,
                               D);
            TBK_HIP(hipGetLastError());
        }
    }
    hipLaunchKernelGGL(trans_lib_check_kernel, grid, dim3(256), 0, s, P, nullptr, n, W.batch, w0, items, n_z, key0, sub_n, sub, d_flag);
    hipLaunchKernelGGL(trans_lib_gamma_kernel, grid, dim3(256), 0, s, es, n, T, P, Q);  // Gamma_R, P_M^H
    TBK_HIP(hipGetLastError());
    TBK_CHECK(surf_lib_gemm(W, T, P, R));  // Gamma_R P_M
    hipLaunchKernelGGL(trans_lib_gamma_kernel, grid, dim3(256), 0, s, et, n, T, nullptr, nullptr);  // Gamma_L
    TBK_HIP(hipGetLastError());
    TBK_CHECK(surf_lib_gemm(W, T, Q, D));  // Gamma_L P_M^H
    hipLaunchKernelGGL(trans_lib_trace_kernel, dim3((unsigned)W.batch), dim3(256), 0, s, R, D, P, n, w0, items, t_stride, t_at, d_T, d_G);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

// The chunk's nkc points at every energy on the library route (the arguments of trans_launch)
int trans_lib_chunk(hipStream_t s, const SurfLib& W, const TransShape& sh, const double2* d_H00, const double2* d_H01, const double2* d_V,
                    const double2* d_z, int64_t nkc, int max_it, int64_t k0, char* d_res) {
    const int n_z = (int)sh.n_z;
    const int64_t items = nkc * sh.n_z;
    const unsigned long long key0 = (unsigned long long)k0 * (unsigned long long)SURF_MAX_Z;
    double* d_T = reinterpret_cast<double*>(d_res);
    int32_t* d_it = reinterpret_cast<int32_t*>(d_res + sh.t_bytes(nkc));
    double2* d_G = sh.green ? reinterpret_cast<double2*>(d_res + sh.t_bytes(nkc) + sh.it_bytes(nkc)) : nullptr;
    unsigned long long* d_flag = reinterpret_cast<unsigned long long*>(d_res + sh.result_bytes(nkc));
    for (int64_t w0 = 0; w0 < items; w0 += W.batch) {
        TBK_CHECK(surf_lib_iterate(s, W, d_H00, d_H01, d_z, n_z, items, w0, max_it, key0, d_it, d_flag));
        TBK_CHECK(trans_lib_sweep(s, W, sh.m_layers, d_H00, d_H01, d_V, d_z, n_z, items, w0, key0, 1ull, 0ull, 1, 0, d_T, d_G, d_flag));
    }
    return TBK_OK;
}

// The ensemble's chunk on the library route (tbk_ensemble.hip has the call): per lockstep batch surf_lib_iterate once, then the sweep
// and the closing per sample -- es and et survive them.  d_V: n_s devices [m_layers][n][n] complex or [m_layers][n] doubles; d_T:
// [nkc][n_z][n_s]; d_flag: the sweeps' word (keys with the sample) and, behind it, the decimation's in surf_lib_norms_kernel's keys.
template <typename VT>
int trans_ens_lib_chunk(hipStream_t s, const SurfLib& W, int m_layers, int64_t n_s, const double2* d_H00, const double2* d_H01, const VT* d_V,
                        const double2* d_z, int64_t n_z, int64_t nkc, int max_it, int64_t k0, int32_t* d_it, double* d_T, unsigned long long* d_flag) {
    const int64_t items = nkc * n_z;
    const unsigned long long key0 = (unsigned long long)k0 * (unsigned long long)SURF_MAX_Z;
    const size_t per_sample = (size_t)m_layers * trans_v_layer(d_V, W.n);
    for (int64_t w0 = 0; w0 < items; w0 += W.batch) {
        TBK_CHECK(surf_lib_iterate(s, W, d_H00, d_H01, d_z, (int)n_z, items, w0, max_it, key0, d_it, d_flag + 1));
        for (int64_t sample = 0; sample < n_s; ++sample)
            TBK_CHECK(trans_lib_sweep(s, W, m_layers, d_H00, d_H01, d_V + (size_t)sample * per_sample, d_z, (int)n_z, items, w0, key0,
                                      (unsigned long long)SURF_MAX_Z, (unsigned long long)sample, n_s, sample, d_T, nullptr, d_flag));
    }
    return TBK_OK;
}

// ---- the two families of this file behind the drivers of tbk_layered.h -----------------------------------------------------------------
// what the library route and the own kernel share of a family: the route's rule and the bytes of either workspace
struct SurfLibFamily : LayeredFamily {
    int rows = 0;
    size_t slot_doubles = 0;  // of a workgroup's slot at NP = 64
    int64_t n_z = 0;
    bool library(int eigensolver) const override { return surf_takes_library(rows, eigensolver); }
    size_t workspace_bytes(bool library, int64_t chunk, int n_cu) const override {
        if (library) return SurfLib::bytes(rows, surf_lib_batch(rows));
        return rows > 32 ? (size_t)surf_grid(rows, chunk * n_z, n_cu) * slot_doubles * sizeof(double) : 0;
    }
    SurfLib placed(const LayeredChunk& c) const {
        SurfLib W;
        W.place(c.d_ws, rows, surf_lib_batch(rows), c.blas);
        return W;
    }
};

struct SurfFamily : SurfLibFamily {
    SurfShape sh;
    int32_t* iterations;
    double *bottom, *top, *bulk;
    SurfFamily(int64_t n_z_, int spectral, int32_t* iterations_, double* bottom_, double* top_, double* bulk_)
        : iterations(iterations_), bottom(bottom_), top(top_), bulk(bulk_) {
        family = needs = SURF_FAMILY;
        timed = TIMED_SURFACE;
        min_layers = 0;
        slot_doubles = SurfGeom<64>::slot_doubles;
        sh.n_z = n_z = n_z_;
        sh.spectral = spectral != 0;
    }
    int check(int N) override {
        sh.n = rows = N;
        TBK_ARG(iterations != nullptr && bottom != nullptr && top != nullptr && bulk != nullptr, "iterations / bottom / top / bulk is NULL");
        return TBK_OK;
    }
    size_t result_bytes(int64_t nk) const override { return sh.result_bytes(nk); }
    int64_t auto_chunk(int64_t nk) const override { return sh.auto_chunk(nk); }
    int run_chunk(bool library, const LayeredChunk& c) const override {
        if (library) return surf_lib_chunk(c.s, placed(c), sh, c.d_H00, c.d_H01, c.d_z, c.nkc, c.max_it, c.k0, c.d_res);
        return surf_launch(c.s, c.n_cu, sh, c.d_H00, c.d_H01, c.d_z, c.nkc, c.max_it, c.k0, reinterpret_cast<double*>(c.d_ws), c.d_res);
    }
    int copy_out(const LayeredCopy& copy, const char* d_res, int64_t nkc, int64_t c0) const override {
        const size_t items = (size_t)nkc * sh.n_z;
        const size_t o = (size_t)c0 * sh.n_z * sh.item_doubles(), ob = items * sh.item_doubles() * sizeof(double);
        TBK_HIP(copy(bottom + o, d_res, ob));
        TBK_HIP(copy(top + o, d_res + sh.out_bytes(nkc), ob));
        TBK_HIP(copy(bulk + o, d_res + 2 * sh.out_bytes(nkc), ob));
        TBK_HIP(copy(iterations + (size_t)c0 * sh.n_z, d_res + 3 * sh.out_bytes(nkc), items * sizeof(int32_t)));
        return TBK_OK;
    }
    int status_error(unsigned long long word, const double* z, int max_iterations) const override {
        return surf_status_error(word, z, max_iterations);
    }
};

struct TransFamily : SurfLibFamily {
    TransShape sh;
    int32_t* iterations;
    double *T, *G;
    TransFamily(int M, const double* V, int64_t n_z_, int32_t* iterations_, double* T_, double* G_) : iterations(iterations_), T(T_), G(G_) {
        family = needs = TRANS_FAMILY;
        timed = TIMED_TRANSMISSION;
        slot_doubles = TransGeom<64>::slot_doubles;
        h_V = V;
        sh.m_layers = M;
        sh.n_z = n_z = n_z_;
        sh.green = G != nullptr;
    }
    int check(int N) override {
        sh.n = rows = N;
        TBK_CHECK(trans_check_device(N, sh.m_layers, static_cast<const double*>(h_V), iterations, T));
        v_bytes = (size_t)sh.m_layers * N * N * sizeof(double2);
        return TBK_OK;
    }
    size_t result_bytes(int64_t nk) const override { return sh.result_bytes(nk); }
    int64_t auto_chunk(int64_t nk) const override { return sh.auto_chunk(nk); }
    int run_chunk(bool library, const LayeredChunk& c) const override {
        const double2* d_V = static_cast<const double2*>(c.d_V);
        if (library) return trans_lib_chunk(c.s, placed(c), sh, c.d_H00, c.d_H01, d_V, c.d_z, c.nkc, c.max_it, c.k0, c.d_res);
        return trans_launch(c.s, c.n_cu, sh, c.d_H00, c.d_H01, d_V, c.d_z, c.nkc, c.max_it, c.k0, reinterpret_cast<double*>(c.d_ws), c.d_res);
    }
    int copy_out(const LayeredCopy& copy, const char* d_res, int64_t nkc, int64_t c0) const override {
        const size_t items = (size_t)nkc * sh.n_z, first = (size_t)c0 * sh.n_z, nn = (size_t)sh.n * sh.n;
        TBK_HIP(copy(T + first, d_res, items * sizeof(double)));
        TBK_HIP(copy(iterations + first, d_res + sh.t_bytes(nkc), items * sizeof(int32_t)));
        if (sh.green) TBK_HIP(copy(G + first * nn * 2, d_res + sh.t_bytes(nkc) + sh.it_bytes(nkc), items * nn * sizeof(double2)));
        return TBK_OK;
    }
    int status_error(unsigned long long word, const double* z, int max_iterations) const override {
        return surf_status_error(word, z, max_iterations, TRANS_SINGULAR);
    }
};

}  // namespace

// tbk_ensemble.hip's doors to the library route: the bytes of its workspace, and a chunk on a workspace of that size
size_t tbk_trans_ens_lib_bytes(int n) { return SurfLib::bytes(n, surf_lib_batch(n)); }

int tbk_trans_ens_lib_chunk(hipStream_t s, rocblas_handle blas, char* d_ws, int n, int m_layers, int64_t n_s, const double2* d_H00, const double2* d_H01,
                            const double2* d_V, const double* d_onsite, const double2* d_z, int64_t n_z, int64_t nkc, int max_it, int64_t k0, int32_t* d_it,
                            double* d_T, unsigned long long* d_flag) {
    SurfLib W;
    W.place(d_ws, n, surf_lib_batch(n), blas);
    if (d_onsite != nullptr) return trans_ens_lib_chunk(s, W, m_layers, n_s, d_H00, d_H01, d_onsite, d_z, n_z, nkc, max_it, k0, d_it, d_T, d_flag);
    return trans_ens_lib_chunk(s, W, m_layers, n_s, d_H00, d_H01, d_V, d_z, n_z, nkc, max_it, k0, d_it, d_T, d_flag);
}

extern "C" int tbk_transmission_from_matrices(int device, int N, int64_t n_k, const double* H00, const double* H01, int M, const double* V, int64_t n_z,
                                              const double* z, int max_iterations, int64_t k_chunk, int32_t* iterations, double* T, double* G) {
    TransFamily fam(M, V, n_z, iterations, T, G);
    return layered_from_matrices(fam, device, N, n_k, H00, H01, n_z, z, max_iterations, k_chunk);
}

// The whole call on one handle; k_base as in tbk_surface_green_slab.
int tbk_transmission_slab(tbk_model* m, int64_t k_base, int axis, int layers, const double* k, int64_t nk, int M_device, const double* V, int64_t n_z,
                          const double* z, int max_iterations, int32_t* iterations, double* T, double* G) {
    TransFamily fam(M_device, V, n_z, iterations, T, G);
    return layered_slab(fam, m, k_base, axis, layers, k, nk, n_z, z, max_iterations);
}

extern "C" int tbk_transmission(tbk_model* m, int axis, int layers, const double* k, int64_t nk, int M, const double* V, int64_t n_z, const double* z,
                                int max_iterations, int32_t* iterations, double* T, double* G) {
    return tbk_transmission_slab(m, 0, axis, layers, k, nk, M, V, n_z, z, max_iterations, iterations, T, G);
}

extern "C" int tbk_transmission_timing(tbk_model* m, double* ms, int64_t* calls, int reset) {
    TBK_ARG(m != nullptr && ms != nullptr && calls != nullptr, "model / ms / calls is NULL");
    return tbk_timed_read(m, TIMED_TRANSMISSION, 3, ms, calls, nullptr, reset);
}

extern "C" int tbk_surface_from_matrices(int device, int N, int64_t n_k, const double* H00, const double* H01, int64_t n_z, const double* z,
                                         int max_iterations, int64_t k_chunk, int spectral, int32_t* iterations, double* bottom, double* top,
                                         double* bulk) {
    SurfFamily fam(n_z, spectral, iterations, bottom, top, bulk);
    return layered_from_matrices(fam, device, N, n_k, H00, H01, n_z, z, max_iterations, k_chunk);
}

// The whole call on one handle; k_base: the index of k[0] in the caller's list (the slabs of tbk_surface_green_multi), for the messages.
int tbk_surface_green_slab(tbk_model* m, int64_t k_base, int axis, int layers, const double* k, int64_t nk, int64_t n_z, const double* z,
                           int max_iterations, int spectral, int32_t* iterations, double* bottom, double* top, double* bulk) {
    SurfFamily fam(n_z, spectral, iterations, bottom, top, bulk);
    return layered_slab(fam, m, k_base, axis, layers, k, nk, n_z, z, max_iterations);
}

extern "C" int tbk_surface_green(tbk_model* m, int axis, int layers, const double* k, int64_t nk, int64_t n_z, const double* z, int max_iterations,
                                 int spectral, int32_t* iterations, double* bottom, double* top, double* bulk) {
    return tbk_surface_green_slab(m, 0, axis, layers, k, nk, n_z, z, max_iterations, spectral, iterations, bottom, top, bulk);
}

extern "C" int tbk_surface_timing(tbk_model* m, double* ms, int64_t* calls, int reset) {
    TBK_ARG(m != nullptr && ms != nullptr && calls != nullptr, "model / ms / calls is NULL");
    return tbk_timed_read(m, TIMED_SURFACE, 3, ms, calls, nullptr, reset);
}
