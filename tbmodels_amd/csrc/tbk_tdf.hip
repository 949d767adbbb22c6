// tbk_tdf.hip -- the transport distribution of a uniform, periodic k mesh by the linear tetrahedron method: the cumulative
// N[a][c](E) = int^E Sigma[a][c] of Sigma[a][c](E) = (1 / NK) sum_k sum_b v_a v_c delta(E - E_kb), from which Boltzmann transport in the
// relaxation-time approximation follows.  Not in the reference; DESIGN.md section 30 has the quantity, the kernels, the error bound and
// the measurements, tools/tdf_model.py is the statement the tests compare with.
//
//   D^a(k)      = (1 / 2 pi) dH/dk_a                                              tbk_chunk_dh: the H(k) kernels on derivative rows
//   V^a(k)      = U^H D^a U                                                       E, U of tbk_eigh_device_rows (convention 2)
//   w[a][c](k, b) = Re sum_{b' : |E_b - E_b'| <= delta} V^a[b][b'] conj(V^c[b][b'])     v_a v_c of an isolated band; summed over a
//                                                                                 degenerate set it is Re tr(P V^a P V^c), whatever
//                                                                                 basis the eigensolver returned inside the set
//
// The accumulation is tbk_pdos.hip's, whose fixed point takes weights in [0, 1].  So the weights kernels write G = dim (dim + 1) / 2
// NON-NEGATIVE channels, each divided by a power of two s_g that the caller derives from the model alone:
//
//   channel a          (a < dim)       sum |V^a[b][b']|^2                         <= B_a^2
//   channel dim + p    (pair p: a < c) sum |V^a[b][b'] + V^c[b][b']|^2            <= (B_a + B_c)^2        pairs (0,1), (0,2), (1,2)
//
// and N[a][c] = (N+[a][c] - N[a][a] - N[c][c]) / 2 is formed from the integrated channels.  A scaled weight above 1 (a scale that is
// too small) is counted per channel in a status word and fails the call; it is never clamped silently.
//
//   tdf_weights_kernel<NP, DIM>   up to 64 orbitals: the geometry of opt_fused_kernel (tbk_optics.hip) -- a workgroup per k-point (four
//                       k-points, a wave each, up to 16 orbitals), U and one D^a staged as swizzled planes in LDS, W = D^a U and
//                       V^a = U^H W on v_mfma_f64_16x16x4_f64 (tbk_velocity.h), V^a of all axes in registers.  The epilogue: a lane
//                       forms the G products of its elements (b, b'), masked by the pair criterion and by the padding, and adds them
//                       over its tiles in tile order; the 16 lanes of a row add theirs in a butterfly (xor 8, 4, 2, 1); the waves
//                       that share a tile row (NP = 32: two) are added in wave order through LDS by the one thread that owns
//                       (b, g) and writes W[k][g][b] = sum / s_g.  The sum is a function of (n, NP) alone; there are no atomics on
//                       floating-point numbers.
//   tdf_weights_global_kernel<DIM>   above 64 orbitals: the products run through rocBLAS (opt_library_rotate) and leave V^a in global
//                       memory; a workgroup per k-point, a wave per row b, lane l the columns l, l + 64, ... in order, then the
//                       wave's butterfly.
//
// W[nk][G][n_orb] of the slab then goes through pdos_launch unchanged (accumulate, reduce, scan: tbk_pdos.hip) with n_groups = G.

#include <algorithm>
#include <cmath>
#include <vector>

#include "tbk_tetra_staged.h"
#include "tbk_velocity.h"

namespace {

constexpr int TDF_THREADS = 256;
constexpr const char* TDF_FAMILY = "the transport distribution";
constexpr const char* TDF_MESH = "the transport distribution needs a 2- or 3-dimensional model";

constexpr int tdf_channels(int dim) { return dim * (dim + 1) / 2; }

// what the weights kernels of a chunk read and write
struct TdfArgs {
    const double* E = nullptr;   // [nkc][n]
    const double2* U = nullptr;  // [nkc][n][n]
    const double2* D = nullptr;  // fused: D^a of point k at D + k d_sk + a d_sa;  global: V^a likewise
    size_t d_sk = 0, d_sa = 0;
    int n = 0;
    int64_t nkc = 0;
    double degeneracy = 0.0;
    const double* inv_scale = nullptr;  // [G] 1 / s_g
    unsigned int* status = nullptr;     // [G] scaled weights above 1 (or not a number)
    double* W = nullptr;                // [nkc][G][n]
};

// the G channel products of one element into sums: |V^a|^2, then |V^a + V^c|^2 for a < c; `keep`: the pair enters
template <int DIM>
__device__ __forceinline__ void tdf_element(bool keep, const double (&vr)[DIM], const double (&vi)[DIM], double (&sum)[DIM * (DIM + 1) / 2]) {
    int p = DIM;
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
        const double d = fma(vr[a], vr[a], vi[a] * vi[a]);
        sum[a] += keep ? d : 0.0;
#pragma unroll
        for (int c = a + 1; c < DIM; ++c) {
            const double sr = vr[a] + vr[c], si = vi[a] + vi[c];
            const double s = fma(sr, sr, si * si);
            sum[p] += keep ? s : 0.0;
            ++p;
        }
    }
}

// one owner's store: the scaled weight, counted when it is not in [0, 1]
__device__ __forceinline__ void tdf_store(const TdfArgs& g, int ch, double sum, double* out) {
    const double scaled = sum * g.inv_scale[ch];
    if (!(scaled <= 1.0)) atomicAdd(&g.status[ch], 1u);
    *out = scaled;
}

// NP: the orbitals padded to 16, 32 or 64.  grid: k-points / KPW.  Dynamic LDS: KPW x [U | D^a or W][Re | Im][NP NP] doubles.
template <int NP, int DIM>
__global__ void __launch_bounds__(TDF_THREADS, NP == 64 ? 1 : 2) tdf_weights_kernel(const TdfArgs g) {
    constexpr int BT = NP / 16;
    constexpr int KPW = BT == 1 ? 4 : 1;     // k-points per workgroup
    constexpr int TEAM = TDF_THREADS / KPW;  // threads that stage one k-point
    constexpr int TPW = BT == 4 ? 4 : 1;     // tiles per wave
    constexpr int PLANE = NP * NP;
    constexpr int G = DIM * (DIM + 1) / 2;
    extern __shared__ __attribute__((aligned(16))) double tdf_lds[];
    __shared__ double row_part[4][G][16];  // the waves' row sums: [wave][channel][row of its tile row]
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int team = KPW == 4 ? wave : 0, tt = tid - team * TEAM;
    const int n = g.n;
    const int64_t k = (int64_t)blockIdx.x * KPW + team;
    const bool valid = k < g.nkc;
    const int64_t ks = valid ? k : 0;
    double* ur = tdf_lds + (size_t)team * 4 * PLANE;
    double *ui = ur + PLANE, *br = ur + 2 * PLANE, *bi = ur + 3 * PLANE;
    // the wave's tiles: <64> tile row `wave`, all four; <32> one of the four; <16> the one tile of its k-point
    const int ti = BT == 4 ? wave : BT == 2 ? wave >> 1 : 0;
    const int tj0 = BT == 2 ? wave & 1 : 0;
    const int steps = (n + 3) / 4;
    const int l15 = lane & 15, lq = lane >> 4;
    // U, once
    opt_stage<NP, TEAM>(g.U + (size_t)ks * n * n, n, valid, tt, ur, ui);
    // the eigenvalues of the lane's rows b and columns b', and the mask of the padding
    double ea[4], eb[TPW];
    bool a_in[4], b_in[TPW];
    {
        const double* Ek = g.E + (size_t)ks * n;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int b = ti * 16 + lq + 4 * r;
            a_in[r] = valid && b < n;
            ea[r] = Ek[a_in[r] ? b : 0];
        }
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
            const int c = (tj0 + t) * 16 + l15;
            b_in[t] = valid && c < n;
            eb[t] = Ek[b_in[t] ? c : 0];
        }
    }
    zd4 vr[DIM][TPW], vi[DIM][TPW];
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
        const double2* Da = g.D + (size_t)ks * g.d_sk + (size_t)a * g.d_sa;
        __syncthreads();  // the previous axis has read its planes (the first: nothing)
        opt_stage<NP, TEAM>(Da, n, valid, tt, br, bi);
        __syncthreads();
        // W = (D^a)^H U = D^a U
        zd4 wr[TPW], wi[TPW];
#pragma unroll
        for (int t = 0; t < TPW; ++t) wr[t] = wi[t] = zd4{0.0, 0.0, 0.0, 0.0};
        opt_product<NP, TPW>(br, bi, ur, ui, steps, ti, tj0, lane, wr, wi);
        __syncthreads();  // every wave has read D^a
#pragma unroll
        for (int t = 0; t < TPW; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int at = opt_at<NP>(ti * 16 + lq + 4 * r, (tj0 + t) * 16 + l15);
                br[at] = wr[t][r];
                bi[at] = wi[t][r];
            }
        __syncthreads();
        // V^a = U^H W
#pragma unroll
        for (int t = 0; t < TPW; ++t) vr[a][t] = vi[a][t] = zd4{0.0, 0.0, 0.0, 0.0};
        opt_product<NP, TPW>(ur, ui, br, bi, steps, ti, tj0, lane, vr[a], vi[a]);
    }
    // the epilogue.  lane (q, c), register r of tile t: row ti 16 + q + 4 r, column (tj0 + t) 16 + c
    const double delta = g.degeneracy;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        double sum[G];
#pragma unroll
        for (int x = 0; x < G; ++x) sum[x] = 0.0;
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
            double er[DIM], ei[DIM];
#pragma unroll
            for (int a = 0; a < DIM; ++a) {
                er[a] = vr[a][t][r];
                ei[a] = vi[a][t][r];
            }
            tdf_element<DIM>(a_in[r] && b_in[t] && fabs(ea[r] - eb[t]) <= delta, er, ei, sum);
        }
        // the 16 lanes of the row (the same q): every one of them ends with the same sum
#pragma unroll
        for (int x = 0; x < G; ++x) {
#pragma unroll
            for (int off = 8; off >= 1; off >>= 1) sum[x] += __shfl_xor(sum[x], off, 64);
            if (l15 == 0) row_part[wave][x][lq + 4 * r] = sum[x];
        }
    }
    __syncthreads();
    // the owners: thread idx one (k-point, channel, row); the waves of a tile row in wave order
    for (int idx = tid; idx < KPW * G * NP; idx += TDF_THREADS) {
        const int kp = idx / (G * NP), rem = idx - kp * (G * NP);
        const int ch = rem / NP, b = rem - ch * NP;
        const int64_t ko = (int64_t)blockIdx.x * KPW + kp;
        if (ko >= g.nkc || b >= n) continue;
        double sum;
        if (BT == 1)
            sum = row_part[kp][ch][b];
        else if (BT == 2)
            sum = row_part[2 * (b >> 4)][ch][b & 15] + row_part[2 * (b >> 4) + 1][ch][b & 15];
        else
            sum = row_part[b >> 4][ch][b & 15];
        tdf_store(g, ch, sum, g.W + ((size_t)ko * G + ch) * n + b);
    }
}

__device__ __forceinline__ double tdf_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// above 64 orbitals: V^a of the chunk in global memory; a workgroup per k-point, wave w the rows w, w + 4, ...
template <int DIM>
__global__ void __launch_bounds__(TDF_THREADS, 2) tdf_weights_global_kernel(const TdfArgs g) {
    constexpr int G = DIM * (DIM + 1) / 2;
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int n = g.n;
    const int64_t k = blockIdx.x;
    const double* Ek = g.E + (size_t)k * n;
    const double2* Vk = g.D + (size_t)k * g.d_sk;
    const double delta = g.degeneracy;
    for (int b = wave; b < n; b += TDF_THREADS / 64) {
        const double e_row = Ek[b];
        double sum[G];
#pragma unroll
        for (int x = 0; x < G; ++x) sum[x] = 0.0;
        for (int c = lane; c < n; c += 64) {
            double er[DIM], ei[DIM];
#pragma unroll
            for (int a = 0; a < DIM; ++a) {
                const double2 v = Vk[(size_t)a * g.d_sa + (size_t)b * n + c];
                er[a] = v.x;
                ei[a] = v.y;
            }
            tdf_element<DIM>(fabs(e_row - Ek[c]) <= delta, er, ei, sum);
        }
#pragma unroll
        for (int x = 0; x < G; ++x) {
            const double total = tdf_wave_sum(sum[x]);
            if (lane == 0) tdf_store(g, x, total, g.W + ((size_t)k * G + x) * n + b);
        }
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
// the fused kernel's template (16, 32, 64), 0: the library route
int tdf_template(int n_orb) { return n_orb <= 16 ? 16 : n_orb <= 32 ? 32 : n_orb <= OPT_FUSED_MAX ? 64 : 0; }

template <int NP, int DIM>
int tdf_launch_fused_as(hipStream_t s, const TdfArgs& a) {
    constexpr int KPW = NP == 16 ? 4 : 1;
    constexpr int lds = KPW * 4 * NP * NP * (int)sizeof(double);
    static tbk_flag_row raised;
    if (lds > 64 * 1024) TBK_HIP(tbk_raise_lds_limit(reinterpret_cast<const void*>(&tdf_weights_kernel<NP, DIM>), lds, raised));
    hipLaunchKernelGGL((tdf_weights_kernel<NP, DIM>), dim3((unsigned)((a.nkc + KPW - 1) / KPW)), dim3(TDF_THREADS), lds, s, a);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

template <int DIM>
int tdf_launch_fused(hipStream_t s, int np, const TdfArgs& a) {
    if (np == 16) return tdf_launch_fused_as<16, DIM>(s, a);
    if (np == 32) return tdf_launch_fused_as<32, DIM>(s, a);
    return tdf_launch_fused_as<64, DIM>(s, a);
}

// The weights of one chunk: `a` as the kernels take it, a.D = D^a of the chunk.  Above 64 orbitals the library's products overwrite
// D^a with V^a first (d_T: [nkc][n][n] complex of scratch); calls stay below 2^29 elements, as those of tbk_eigh.
int tdf_launch_weights(hipStream_t s, rocblas_handle blas, int dim, const TdfArgs& a, double* d_T) {
    if (tdf_template(a.n) != 0) return dim == 2 ? tdf_launch_fused<2>(s, tdf_template(a.n), a) : tdf_launch_fused<3>(s, tdf_template(a.n), a);
    typedef rocblas_double_complex Z;
    const int64_t nn = (int64_t)a.n * a.n, step = std::max<int64_t>(1, (int64_t(1) << 29) / nn);
    for (int ax = 0; ax < dim; ++ax)
        for (int64_t b0 = 0; b0 < a.nkc; b0 += step) {
            const rocblas_int nb = (rocblas_int)std::min(step, a.nkc - b0);
            const Z* Uc = reinterpret_cast<const Z*>(a.U) + (size_t)b0 * nn;
            Z* Da = reinterpret_cast<Z*>(const_cast<double2*>(a.D)) + (size_t)b0 * a.d_sk + (size_t)ax * a.d_sa;
            TBK_CHECK(opt_library_rotate(blas, a.n, nb, Uc, Da, a.d_sk, reinterpret_cast<Z*>(d_T) + (size_t)b0 * nn));
        }
    if (dim == 2)
        hipLaunchKernelGGL((tdf_weights_global_kernel<2>), dim3((unsigned)a.nkc), dim3(TDF_THREADS), 0, s, a);
    else
        hipLaunchKernelGGL((tdf_weights_global_kernel<3>), dim3((unsigned)a.nkc), dim3(TDF_THREADS), 0, s, a);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

// the scales and the status words of a call in one small buffer: 1 / s_g [8], then the counters [8]
constexpr size_t TDF_STATUS_OFF = 8 * sizeof(double);
constexpr size_t TDF_CONST_BYTES = TDF_STATUS_OFF + 8 * sizeof(unsigned int);

struct TdfConst {
    double inv[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    void set(int dim, const double* scale) {
        for (int g = 0; g < tdf_channels(dim); ++g) inv[g] = 1.0 / scale[g];
    }
    int upload(void* d, hipStream_t s) const {
        TBK_HIP(hipMemcpyAsync(d, inv, sizeof(inv), hipMemcpyHostToDevice, s));
        TBK_HIP(hipMemsetAsync(static_cast<char*>(d) + TDF_STATUS_OFF, 0, 8 * sizeof(unsigned int), s));
        return TBK_OK;
    }
};

// the counters after the stream has been waited for: the first channel with a weight above 1 fails the call
int tdf_check_status(const void* d_const, int dim) {
    unsigned int count[8];
    TBK_HIP(hipMemcpy(count, static_cast<const char*>(d_const) + TDF_STATUS_OFF, sizeof(count), hipMemcpyDeviceToHost));
    for (int g = 0; g < tdf_channels(dim); ++g)
        if (count[g] != 0) {
            tbk_set_error("invalid argument: %u scaled weights of channel %d of the transport distribution are above 1: scale[%d] is too small", count[g], g, g);
            return TBK_ERR_ARGUMENT;
        }
    return TBK_OK;
}

}  // namespace

int tbk_tdf_check_arguments(int dim, double degeneracy, const double* scale) {
    TBK_ARG(dim == 2 || dim == 3, TDF_MESH);
    TBK_ARG(std::isfinite(degeneracy) && degeneracy >= 0.0, "degeneracy is negative or not finite");
    TBK_ARG(scale != nullptr, "scale is NULL");
    for (int g = 0; g < tdf_channels(dim); ++g) TBK_ARG(std::isfinite(scale[g]) && scale[g] > 0.0, "a scale is not positive and finite");
    return TBK_OK;
}

extern "C" int tbk_tdf_weights_from_eigensystem(int device, int dim, int n_orb, int64_t nk, const double* E, const double* U, const double* D,
                                                double degeneracy, const double* scale, double* W_out) {
    TBK_CHECK(tbk_tdf_check_arguments(dim, degeneracy, scale));
    TBK_ARG(n_orb >= 1 && nk >= 1 && nk <= (int64_t(1) << 23), "n_orb / nk < 1 or more than 2^23 points");
    TBK_ARG(E != nullptr && U != nullptr && D != nullptr && W_out != nullptr, "E / U / D / W is NULL");
    TBK_CHECK(tetra_check_device(device));
    const int G = tdf_channels(dim);
    const size_t nn = (size_t)n_orb * n_orb;
    const size_t e_bytes = (size_t)nk * n_orb * sizeof(double), u_bytes = (size_t)nk * nn * sizeof(double2);
    DevBuf d_E, d_U, d_D, d_T, d_W, d_const;
    Owned<rocblas_handle, rocblas_destroy_handle> blas;
    TBK_CHECK(d_E.reserve(e_bytes));
    TBK_CHECK(mesh_reserve(d_U, u_bytes, TDF_FAMILY, "the eigenvectors"));
    TBK_CHECK(mesh_reserve(d_D, u_bytes * dim, TDF_FAMILY, "the derivatives"));
    TBK_CHECK(d_W.reserve(e_bytes * G));
    TBK_CHECK(d_const.reserve(TDF_CONST_BYTES));
    if (tdf_template(n_orb) == 0) {
        TBK_CHECK(mesh_reserve(d_T, u_bytes, TDF_FAMILY, "the library's products"));
        TBK_ROCBLAS(rocblas_create_handle(blas.put()));
    }
    TdfConst h;
    h.set(dim, scale);
    TBK_CHECK(h.upload(d_const.ptr, nullptr));
    TBK_HIP(hipMemcpy(d_E.ptr, E, e_bytes, hipMemcpyHostToDevice));
    TBK_HIP(hipMemcpy(d_U.ptr, U, u_bytes, hipMemcpyHostToDevice));
    TBK_HIP(hipMemcpy(d_D.ptr, D, u_bytes * dim, hipMemcpyHostToDevice));
    TdfArgs a;
    a.E = d_E.as<double>();
    a.U = d_U.as<double2>();
    a.D = d_D.as<double2>();
    a.d_sk = nn * dim;
    a.d_sa = nn;
    a.n = n_orb;
    a.nkc = nk;
    a.degeneracy = degeneracy;
    a.inv_scale = d_const.as<double>();
    a.status = reinterpret_cast<unsigned int*>(d_const.as<char>() + TDF_STATUS_OFF);
    a.W = d_W.as<double>();
    TBK_CHECK(tdf_launch_weights(nullptr, blas, dim, a, d_T.as<double>()));
    TBK_HIP(hipMemcpy(W_out, d_W.ptr, e_bytes * G, hipMemcpyDeviceToHost));
    return tdf_check_status(d_const.ptr, dim);
}

namespace {

struct TdfSlab {
    int mode = TBK_TDF_WHOLE;
    double* h_E = nullptr;  // TBK_TDF_WEIGHTS: where E and W of the slab's own planes go; TBK_TDF_ACCUMULATE: E and W of the whole mesh
    double* h_W = nullptr;
    size_t ws_bytes = 0;
    double* d_W = nullptr;
};

// The reservations of one slab and, enqueued, E and W of its planes (pdos_fill's shape).  E goes to ws_out and W to ws_pdos_w for the
// planes of the slab and its periodic neighbour plane; the eigenvectors (ws_pdos_u), the derivatives (ws_dm_p) and above 64 orbitals
// the library's scratch (ws_mesh_work) exist one k chunk at a time.  E, U come from tbk_eigh_device_rows with caller_rows, the call
// tbk_optics.hip walks with: every chunk stays on the H(k) paths that read finished phase rows, so that no bit of a k-point knows
// the length of its chunk (up to tbk_hk_stable_chunk points).  All reservations stand before the first fill.
// TBK_TDF_WEIGHTS: the slab's own planes alone, E and W copied to the host behind the walk and nothing reserved for the accumulation;
// TBK_TDF_ACCUMULATE: no walk, E and W of the whole mesh come from the host.
int tdf_fill(const TetraStaged& t, TetraSlab& s, const int32_t* mesh, int64_t n_e, double degeneracy, const TdfConst& h, TdfSlab* out) {
    tbk_model* m = s.m;
    const int dim = t.dim, n = t.n_orb, G = tdf_channels(dim);
    const int64_t planes = out->mode == TBK_TDF_WEIGHTS ? s.p_count : s.planes;
    const int64_t nk = planes * t.plane_pts;
    const size_t nn = (size_t)n * n;
    const bool library = tdf_template(n) == 0;
    const size_t e_bytes = (size_t)nk * n * sizeof(double);
    if (out->mode != TBK_TDF_WEIGHTS) TBK_CHECK(tbk_pdos_weighted_bytes(dim, mesh, s.p_count, s.planes, n, G, n_e, &out->ws_bytes));
    TBK_CHECK(tbk_dos_mesh_klist(dim, mesh, s.p_lo, planes, &s.h_k));
    const size_t k_bytes = s.h_k.size() * sizeof(double);
    const size_t nos_bytes = (size_t)G * (size_t)n_e * sizeof(double);
    // what stays for the whole call first, so that the chunk is chosen from what is left
    TBK_CHECK(m->ws_k.reserve(k_bytes));
    TBK_CHECK(mesh_reserve(m->ws_out, e_bytes, TDF_FAMILY, "the eigenvalues of the slab"));
    TBK_CHECK(mesh_reserve(m->ws_pdos_w, e_bytes * G, TDF_FAMILY, "the weights of the slab"));
    TBK_CHECK(m->ws_pdos_grp.reserve(TDF_CONST_BYTES));
    if (out->mode != TBK_TDF_WEIGHTS) TBK_CHECK(m->ws_dos.reserve(out->ws_bytes + dos_align256(nos_bytes)));
    out->d_W = m->ws_pdos_w.as<double>();
    s.d_E = m->ws_out.as<double>();
    if (out->mode == TBK_TDF_ACCUMULATE) {
        TBK_CHECK(h.upload(m->ws_pdos_grp.ptr, m->stream));  // (the status words: zeros)
        TBK_HIP(hipMemcpyAsync(m->ws_out.ptr, out->h_E, e_bytes, hipMemcpyHostToDevice, m->stream));
        TBK_HIP(hipMemcpyAsync(m->ws_pdos_w.ptr, out->h_W, e_bytes * G, hipMemcpyHostToDevice, m->stream));
        return TBK_OK;
    }
    // the chunk of the eigenvector walk: beside U the dim derivatives (the library route: its scratch too), as tbk_optics.hip's
    int64_t chunk = mesh_eigh_chunk(m, nk, 1 + dim + (library ? 1 : 0));
    if (tbk_hk_stable_chunk(m) > 0) chunk = std::min(chunk, tbk_hk_stable_chunk(m));
    const size_t u_bytes = (size_t)chunk * nn * sizeof(double2);
    TBK_CHECK(mesh_reserve(m->ws_pdos_u, u_bytes, TDF_FAMILY, "the eigenvectors of one chunk"));
    TBK_CHECK(mesh_reserve(m->ws_dm_p, u_bytes * dim, TDF_FAMILY, "the derivatives of one chunk"));
    if (library) {
        TBK_CHECK(mesh_reserve(m->ws_mesh_work, u_bytes, TDF_FAMILY, "the library's products of one chunk"));
        m->counters[TBK_CNT_LIBRARY_CALLS] += 1;
    }
    TBK_HIP(hipMemcpyAsync(m->ws_k.ptr, s.h_k.data(), k_bytes, hipMemcpyHostToDevice, m->stream));
    TBK_CHECK(h.upload(m->ws_pdos_grp.ptr, m->stream));

    const double* d_k = m->ws_k.as<double>();
    double* d_E = m->ws_out.as<double>();
    double* d_U = m->ws_pdos_u.as<double>();
    for (int64_t c0 = 0; c0 < nk; c0 += chunk) {
        const int64_t nkc = std::min(chunk, nk - c0);
        TBK_CHECK(tbk_eigh_device_rows(m, d_k + c0 * dim, nkc, 2, nullptr, d_E + c0 * n, d_U, true));
        s.ev->start(0);
        int status = TBK_OK;
        for (int a = 0; a < dim && status == TBK_OK; ++a)
            status = tbk_chunk_dh(m, a, d_k + c0 * dim, nkc, m->ws_dm_p.as<double>() + (size_t)a * nkc * nn * 2);
        s.ev->stop();  // (before the status is looked at: no span stays open)
        TBK_CHECK(status);
        TdfArgs a;
        a.E = d_E + c0 * n;
        a.U = reinterpret_cast<const double2*>(d_U);
        a.D = m->ws_dm_p.as<double2>();
        a.d_sk = nn;
        a.d_sa = (size_t)nkc * nn;
        a.n = n;
        a.nkc = nkc;
        a.degeneracy = degeneracy;
        a.inv_scale = m->ws_pdos_grp.as<double>();
        a.status = reinterpret_cast<unsigned int*>(m->ws_pdos_grp.as<char>() + TDF_STATUS_OFF);
        a.W = out->d_W + (size_t)c0 * G * n;
        s.ev->start(1);
        status = tdf_launch_weights(m->stream, library ? (rocblas_handle)m->blas : nullptr, dim, a, m->ws_mesh_work.as<double>());
        s.ev->stop();
        TBK_CHECK(status);
    }
    if (out->mode == TBK_TDF_WEIGHTS) {
        TBK_HIP(hipMemcpyAsync(out->h_E, d_E, e_bytes, hipMemcpyDeviceToHost, m->stream));
        TBK_HIP(hipMemcpyAsync(out->h_W, out->d_W, e_bytes * G, hipMemcpyDeviceToHost, m->stream));
    }
    return TBK_OK;
}

}  // namespace

// Cells [p_lo, p_lo + p_count) along axis 0 of the mesh on one handle: a one-slab case of the scaffold (tbk_tetra_staged.h) with
// tdf_fill as its reservation step, tbk_pdos_slab's shape.  TBK_TDF_WHOLE (the whole axis): cumulative_out[G][n_e] -- the caller's, it
// outlives the wait -- receives the channels, divided by S * NK and multiplied back by the scales (powers of two: exactly).  The two
// halves of a call on several handles: TBK_TDF_WEIGHTS leaves E[points][n] and W[points][G][n] of the slab's own planes in h_E and h_W
// (the caller's, at the slab's place in the mesh), TBK_TDF_ACCUMULATE (the whole axis) takes E and W of the whole mesh from there and
// runs the accumulation alone -- on one handle, because the fixed-point sums of slabs, once divided and rounded, do not add up to
// the bits of one launch.  The recorder's stages: 0 the derivative contractions, 1 the weights kernel (the library's products
// included), 2 accumulate, reduction and scan (pdos_launch books them on a recorder of its own, whose two rows are added here).
int tbk_tdf_slab(tbk_model* m, const int32_t* mesh, int64_t p_lo, int64_t p_count, double e_min, double e_step, int64_t n_e, double degeneracy,
                 const double* scale, int mode, double* h_E, double* h_W, double* cumulative_out) {
    TBK_ARG(m != nullptr, "model is NULL");
    TBK_ARG(!m->kdotp, "a k.p model has no Brillouin zone");
    TBK_CHECK(tbk_tdf_check_arguments(m->dim, degeneracy, scale));
    int64_t nk_total = 0;
    TBK_CHECK(tbk_dos_check(m->dim, mesh, e_step, n_e, cumulative_out, &nk_total));
    TBK_ARG(std::isfinite(e_min), "e_min is not finite");
    TBK_ARG(p_lo >= 0 && p_count >= 1 && p_lo + p_count <= mesh[0], "slab outside the mesh");
    TBK_ARG(mode == TBK_TDF_WEIGHTS || (p_lo == 0 && p_count == mesh[0]), "the accumulation takes the whole mesh");
    TBK_ARG(mode == TBK_TDF_WHOLE || (h_E != nullptr && h_W != nullptr), "E / W is NULL");
    const int G = tdf_channels(m->dim);
    // (the source of an enqueued copy and the recorder of the last launches: in front of `staged`, which waits before they go)
    TdfConst h;
    h.set(m->dim, scale);
    SpanRecorder tail(m->timing, m->stream);
    TdfSlab own;
    own.mode = mode;
    own.h_E = h_E;
    own.h_W = h_W;
    TetraStaged staged;
    TBK_CHECK(staged.make_slab(
        m, mesh, TDF_MESH, p_lo, p_count, [&](TetraSlab& s, size_t) { return tdf_fill(staged, s, mesh, n_e, degeneracy, h, &own); }, true));
    if (mode == TBK_TDF_WEIGHTS) {
        TBK_CHECK(staged.streams.book(TIMED_TDF));
        return tdf_check_status(m->ws_pdos_grp.ptr, staged.dim);
    }
    const TetraSlab& s = staged.slabs[0];
    const size_t bins = (size_t)G * (size_t)n_e;
    double* d_nos = reinterpret_cast<double*>(m->ws_dos.as<char>() + own.ws_bytes);
    TBK_CHECK(tbk_pdos_weighted_launch(m->stream, staged.dim, mesh, s.p_count, s.planes, staged.n_orb, G, n_e, s.d_E, own.d_W, e_min, e_step,
                                       (double)(staged.dim == 3 ? 6 : 2) * (double)nk_total, m->ws_dos.ptr, d_nos, tail));
    TBK_HIP(hipMemcpyAsync(cumulative_out, d_nos, bins * sizeof(double), hipMemcpyDeviceToHost, m->stream));
    if (mode == TBK_TDF_WHOLE)
        TBK_CHECK(staged.streams.book(TIMED_TDF));
    else
        TBK_HIP(hipStreamSynchronize(m->stream));  // (the call was booked with the handle's weights)
    double last[3] = {0.0, 0.0, 0.0};
    tail.collect(last);
    m->timed[TIMED_TDF].ms[2] += last[1] + last[2];
    if (mode == TBK_TDF_WHOLE) TBK_CHECK(tdf_check_status(m->ws_pdos_grp.ptr, staged.dim));
    for (int g = 0; g < G; ++g)
        for (int64_t j = 0; j < n_e; ++j) cumulative_out[(size_t)g * n_e + j] *= scale[g];
    return TBK_OK;
}

extern "C" int tbk_transport_distribution(tbk_model* m, const int32_t* mesh, double e_min, double e_step, int64_t n_e, double degeneracy,
                                          const double* scale, double* cumulative_out) {
    TBK_ARG(m != nullptr, "model is NULL");
    TBK_ARG(!m->kdotp, "a k.p model has no Brillouin zone");
    TBK_ARG(mesh != nullptr && cumulative_out != nullptr, "mesh / cumulative is NULL");
    TBK_CHECK(tbk_tdf_check_arguments(m->dim, degeneracy, scale));
    TBK_ARG(mesh[0] >= 1, "a mesh entry is < 1");
    return tbk_tdf_slab(m, mesh, 0, mesh[0], e_min, e_step, n_e, degeneracy, scale, TBK_TDF_WHOLE, nullptr, nullptr, cumulative_out);
}

extern "C" int tbk_tdf_timing(tbk_model* m, double* ms, int64_t* calls, int reset) {
    TBK_ARG(m != nullptr && ms != nullptr && calls != nullptr, "model / ms / calls is NULL");
    return tbk_timed_read(m, TIMED_TDF, 3, ms, calls, nullptr, reset);
}
