// tbk_optics.hip -- the Kubo optical (current-current) conductivity sigma[a][c](omega + i eta) of a uniform, periodic k mesh at one
// chemical potential and one temperature.  Not in the reference; DESIGN.md section 27 has the quantity, the kernels, the error bound
// and the measurements, tools/optics_model.py is the statement the tests compare with.
//
//   D^a(k)      = (1 / 2 pi) dH/dk_a = sum_R i R_a exp(2 pi i k.R) hop[R] + h.c.        tbk_chunk_dh: the H(k) kernels on derivative rows
//   V^a(k)      = U^H D^a U  (+ i (E_b - E_b') (U^H diag(pos[:, a]) U)[b][b'] for convention 1)      E, U of tbk_eigh_device_rows
//   t[b][b']    = f(E_b) (1 - f(E_b')) h((lo - hi) / T) >= 0                               chi_pair_weight (tbk_pair.h): w = t / T
//   sigma[a][c](omega) = (i / (T NK)) sum_k sum_{b b'} t V^a[b][b'] conj(V^c[b][b']) / (omega + i eta + E_b - E_b')
//
// The mesh is walked in chunks of eigenvectors; nothing of the size of the mesh but the partial sums stays on the device, and only
// NW dim^2 complex numbers come back.
//
//   opt_fused_kernel<NP, DIM>  up to 64 orbitals, a workgroup per k-point (four k-points, a wave each, up to 16 orbitals).  U and one
//                       D^a are staged as planes Re / Im in LDS (NP x NP doubles each, padded with zeros; rows of 32 or 64 doubles
//                       are stored with column c ^ 16 in the odd rows, so that the two rows a ds_read_b64 group of 32 lanes reads land
//                       in different halves of the banks).  W = D^a U = (D^a)^H U and V^a = U^H W are the same real products on
//                       v_mfma_f64_16x16x4_f64 -- Mr = Xr^T Yr + Xi^T Yi, Mi = Xr^T Yi - Xi^T Yr (the minus is the negate-A bit) --
//                       and W takes D^a's place in LDS between them; convention 1 adds U^H (pos_a o U), the rows scaled while
//                       staging.  V^a is never stored: a lane keeps its elements of all DIM axes in registers, with t and the
//                       eigenvalues of their rows and columns, and walks the frequencies in chunks of WC.
//   opt_global_kernel<DIM>  above 64 orbitals: the two (three) products run through rocblas_zgemm_strided_batched into a V buffer of
//                       the chunk, and the same epilogue walks it from global memory, 256 elements at a time.
//   opt_element         the epilogue of one pair of states and one chunk of frequencies: p[a][c] = t V^a conj(V^c) for a <= c, x = Delta
//                       + omega, r = (x - i eta) / (x^2 + eta^2), S[a][c] += p r and S[c][a] += conj(p) r.  Every frequency of a chunk
//                       runs the same instructions on its own accumulators (a short chunk is filled up with copies of its last
//                       frequency, which are not stored), so the bits of one frequency do not know its place in the chunk, the pass or
//                       the list.  The lane's elements, then the wave's lanes, then the block's waves: one complex partial per
//                       (k, omega, a, c) in part[k][omega][a][c].
//   opt_group_kernel    the partials of 256 consecutive mesh points, in index order: groups[g][omega][a][c].
//   opt_final_kernel    the groups in index order; sigma = i S / T / NK as differences from +0, so that zeros of either sign give +0.
//
// The partials of all frequencies take 16 dim^2 NW NK bytes; when they do not fit the budget the frequencies go in passes (whole
// register chunks when one fits) and every pass walks the mesh again.  Handles take whole groups, so the sum is the same sum whatever
// their number: the group sums of the later handles are copied to the first, which adds them all up.  No atomics anywhere.

#include <algorithm>
#include <cmath>
#include <vector>

#include "tbk_occ.h"
#include "tbk_pair.h"
#include "tbk_velocity.h"

namespace {

constexpr int OPT_THREADS = PAIR_THREADS;
constexpr int OPT_GROUP = 256;                          // mesh points per summation group
constexpr size_t OPT_PART_BUDGET = size_t(1) << 30;     // the partials of one pass, at most
constexpr int64_t OPT_MAX_NW = int64_t(1) << 23;
constexpr int64_t OPT_MAX_NK = int64_t(1) << 23;
constexpr const char* OPT_FAMILY = "the optical conductivity";

// frequencies per register chunk: 2 DIM^2 WC accumulators per lane, beside the 8 DIM doubles of V^a per tile the lane holds (longer
// chunks spilled: DESIGN.md 27.3)
template <int DIM>
constexpr int opt_wc() {
    return DIM == 2 ? 4 : 2;
}

// one pair of states, one chunk of frequencies.  acc[j][(a DIM + c) 2 + (0: Re, 1: Im)] of S[a][c] = sum p[a][c] r
template <int DIM, int WC>
__device__ __forceinline__ void opt_element(double t, const double (&vr)[DIM], const double (&vi)[DIM], double delta, const double (&om)[WC],
                                            double eta, double eta2, double (&acc)[WC][DIM * DIM * 2]) {
    double pr[DIM][DIM], pi[DIM][DIM];  // a <= c; the diagonal is real: t |V^a|^2
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
        const double tr = t * vr[a], ti = t * vi[a];
#pragma unroll
        for (int c = a; c < DIM; ++c) {
            pr[a][c] = fma(tr, vr[c], ti * vi[c]);
            pi[a][c] = fma(ti, vr[c], -(tr * vi[c]));
        }
    }
#pragma unroll
    for (int j = 0; j < WC; ++j) {
        const double x = delta + om[j];
        const double d = 1.0 / fma(x, x, eta2);
        const double rr = x * d, ri = -(eta * d);
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
            acc[j][(a * DIM + a) * 2] = fma(pr[a][a], rr, acc[j][(a * DIM + a) * 2]);
            acc[j][(a * DIM + a) * 2 + 1] = fma(pr[a][a], ri, acc[j][(a * DIM + a) * 2 + 1]);
#pragma unroll
            for (int c = a + 1; c < DIM; ++c) {
                // p r = (pr rr - pi ri) + i (pr ri + pi rr);  conj(p) r = (pr rr + pi ri) + i (pr ri - pi rr)
                const double m1 = pr[a][c] * rr, m2 = pi[a][c] * ri, m3 = pr[a][c] * ri, m4 = pi[a][c] * rr;
                acc[j][(a * DIM + c) * 2] += m1 - m2;
                acc[j][(a * DIM + c) * 2 + 1] += m3 + m4;
                acc[j][(c * DIM + a) * 2] += m1 + m2;
                acc[j][(c * DIM + a) * 2 + 1] += m3 - m4;
            }
        }
    }
}

// what every kernel of a chunk reads
struct OptArgs {
    const double* E = nullptr;     // [nkc][n]
    const double* tab = nullptr;   // f, 1 - f of the chunk: [2][nkc n]
    const double2* U = nullptr;    // [nkc][n][n]
    const double2* D = nullptr;    // fused: D^a of point k at D + k d_sk + a d_sa;  global: V^a likewise
    const double2* P = nullptr;    // global, convention 1: U^H diag(pos_a) U likewise
    size_t d_sk = 0, d_sa = 0;
    const double* pos = nullptr;   // fused, convention 1: [n][DIM]
    int n = 0;
    int64_t nkc = 0;
    double inv_t = 0.0;
    const double* W = nullptr;     // the frequencies of this pass [nw]
    int nw = 0;
    double eta = 0.0;
    double* part = nullptr;        // [points of the slab][nw][DIM DIM] complex
    int64_t k_off = 0;             // the chunk's first point in part
};

// (opt_at and opt_product -- the planes and the product of two staged matrices -- are tbk_velocity.h's.  The staging loops below stay
// written out: through the header's opt_stage the fused kernels compile to other instruction streams)

// the wave's sums of one chunk of frequencies into part: KPW == 4, a wave per k-point, lane 0 writes; else the block's four waves are
// added in order through LDS
template <int DIM, int WC, int KPW>
__device__ __forceinline__ void opt_store_chunk(double (&acc)[WC][DIM * DIM * 2], double (*wave_acc)[WC][DIM * DIM * 2], const OptArgs& g, int64_t k,
                                                bool valid, int w0, int tid) {
    constexpr int D2 = DIM * DIM * 2;
    const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int j = 0; j < WC; ++j)
#pragma unroll
        for (int x = 0; x < D2; ++x) acc[j][x] = chi_wave_sum(acc[j][x]);
    if (KPW == 4) {
        if (valid && lane == 0) {
#pragma unroll
            for (int j = 0; j < WC; ++j)
                if (w0 + j < g.nw) {
                    double* out = g.part + (((size_t)(g.k_off + k) * g.nw + (w0 + j)) * D2);
#pragma unroll
                    for (int x = 0; x < D2; ++x) out[x] = acc[j][x];
                }
        }
    } else {
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < WC; ++j)
#pragma unroll
                for (int x = 0; x < D2; ++x) wave_acc[wave][j][x] = acc[j][x];
        }
        __syncthreads();
        if (tid < WC * D2) {
            const int j = tid / D2, x = tid - j * D2;
            if (w0 + j < g.nw)
                g.part[((size_t)(g.k_off + k) * g.nw + (w0 + j)) * D2 + x] =
                    ((wave_acc[0][j][x] + wave_acc[1][j][x]) + wave_acc[2][j][x]) + wave_acc[3][j][x];
        }
        __syncthreads();  // (the next chunk writes wave_acc)
    }
}

// NP: the orbitals padded to 16, 32 or 64.  grid: k-points / KPW.  Dynamic LDS: KPW x [U | D^a or W][Re | Im][NP NP] doubles.
template <int NP, int DIM>
__global__ void __launch_bounds__(OPT_THREADS, NP == 64 ? 1 : 2) opt_fused_kernel(const OptArgs g) {
    constexpr int BT = NP / 16;
    constexpr int KPW = BT == 1 ? 4 : 1;     // k-points per workgroup
    constexpr int TEAM = OPT_THREADS / KPW;  // threads that stage one k-point
    constexpr int TPW = BT == 4 ? 4 : 1;     // tiles per wave
    constexpr int WC = opt_wc<DIM>();
    constexpr int PLANE = NP * NP;
    extern __shared__ __attribute__((aligned(16))) double opt_lds[];
    __shared__ double wave_acc[4][WC][DIM * DIM * 2];
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int team = KPW == 4 ? wave : 0, tt = tid - team * TEAM;
    const int n = g.n;
    const int64_t k = (int64_t)blockIdx.x * KPW + team;
    const bool valid = k < g.nkc;
    const int64_t ks = valid ? k : 0;
    double* ur = opt_lds + (size_t)team * 4 * PLANE;
    double *ui = ur + PLANE, *br = ur + 2 * PLANE, *bi = ur + 3 * PLANE;
    const double2* Uk = g.U + (size_t)ks * n * n;
    // the wave's tiles: <64> tile row `wave`, all four; <32> one of the four; <16> the one tile of its k-point
    const int ti = BT == 4 ? wave : BT == 2 ? wave >> 1 : 0;
    const int tj0 = BT == 2 ? wave & 1 : 0;
    const int steps = (n + 3) / 4;
    const int l15 = lane & 15, lq = lane >> 4;
    // U, once
    for (int idx = tt; idx < PLANE; idx += TEAM) {
        const int o = idx / NP, c = idx - o * NP;
        double2 v = make_double2(0.0, 0.0);
        if (valid && o < n && c < n) v = Uk[(size_t)o * n + c];
        ur[opt_at<NP>(o, c)] = v.x;
        ui[opt_at<NP>(o, c)] = v.y;
    }
    // the eigenvalues and the table entries of the lane's rows b and columns b', and the mask of the padding
    double ea[4], fa[4], ga[4], eb[TPW], fb[TPW], gb[TPW];
    bool a_in[4], b_in[TPW];
    {
        const double* Ek = g.E + (size_t)ks * n;
        const double *fk = g.tab + (size_t)ks * n, *gk = fk + (size_t)g.nkc * n;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int b = ti * 16 + lq + 4 * r;
            a_in[r] = valid && b < n;
            const int bs = a_in[r] ? b : 0;
            ea[r] = Ek[bs];
            fa[r] = fk[bs];
            ga[r] = gk[bs];
        }
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
            const int c = (tj0 + t) * 16 + l15;
            b_in[t] = valid && c < n;
            const int cs = b_in[t] ? c : 0;
            eb[t] = Ek[cs];
            fb[t] = fk[cs];
            gb[t] = gk[cs];
        }
    }
    zd4 vr[DIM][TPW], vi[DIM][TPW];
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
        const double2* Da = g.D + (size_t)ks * g.d_sk + (size_t)a * g.d_sa;
        __syncthreads();  // the previous axis has read its planes (the first: nothing)
        for (int idx = tt; idx < PLANE; idx += TEAM) {
            const int o = idx / NP, c = idx - o * NP;
            double2 v = make_double2(0.0, 0.0);
            if (valid && o < n && c < n) v = Da[(size_t)o * n + c];
            br[opt_at<NP>(o, c)] = v.x;
            bi[opt_at<NP>(o, c)] = v.y;
        }
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
        if (g.pos != nullptr) {
            // convention 1: V^a += i (E_b - E_b') (U^H (pos_a o U))[b][b'], the rows of U scaled while staging
            __syncthreads();  // every wave has read W
            for (int idx = tt; idx < PLANE; idx += TEAM) {
                const int o = idx / NP, c = idx - o * NP;
                double2 v = make_double2(0.0, 0.0);
                if (valid && o < n && c < n) {
                    const double p = g.pos[(size_t)o * DIM + a];
                    v = Uk[(size_t)o * n + c];
                    v = make_double2(p * v.x, p * v.y);
                }
                br[opt_at<NP>(o, c)] = v.x;
                bi[opt_at<NP>(o, c)] = v.y;
            }
            __syncthreads();
#pragma unroll
            for (int t = 0; t < TPW; ++t) wr[t] = wi[t] = zd4{0.0, 0.0, 0.0, 0.0};
            opt_product<NP, TPW>(ur, ui, br, bi, steps, ti, tj0, lane, wr, wi);
#pragma unroll
            for (int t = 0; t < TPW; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double de = ea[r] - eb[t];
                    vr[a][t][r] = fma(-de, wi[t][r], vr[a][t][r]);
                    vi[a][t][r] = fma(de, wr[t][r], vi[a][t][r]);
                }
        }
    }
    // the epilogue.  lane (q, c), register r of tile t: row ti 16 + q + 4 r, column (tj0 + t) 16 + c
    double tw[TPW][4];
#pragma unroll
    for (int t = 0; t < TPW; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            tw[t][r] = (a_in[r] && b_in[t]) ? chi_pair_weight(ea[r], fa[r], ga[r], eb[t], fb[t], gb[t], g.inv_t) : 0.0;
    const double eta = g.eta, eta2 = eta * eta;
    for (int w0 = 0; w0 < g.nw; w0 += WC) {
        double om[WC], acc[WC][DIM * DIM * 2];
#pragma unroll
        for (int j = 0; j < WC; ++j) {
            om[j] = g.W[w0 + j < g.nw ? w0 + j : g.nw - 1];  // (uniform; beyond the list: computed, not stored)
#pragma unroll
            for (int x = 0; x < DIM * DIM * 2; ++x) acc[j][x] = 0.0;
        }
#pragma unroll
        for (int t = 0; t < TPW; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double er[DIM], ei[DIM];
#pragma unroll
                for (int a = 0; a < DIM; ++a) {
                    er[a] = vr[a][t][r];
                    ei[a] = vi[a][t][r];
                }
                opt_element<DIM, WC>(tw[t][r], er, ei, ea[r] - eb[t], om, eta, eta2, acc);
            }
        opt_store_chunk<DIM, WC, KPW>(acc, wave_acc, g, k, valid, w0, tid);
    }
}

// above 64 orbitals: V^a (and P^a) of the chunk in global memory; a workgroup per k-point, thread t the elements t, t + 256, ...
template <int DIM>
__global__ void __launch_bounds__(OPT_THREADS, 2) opt_global_kernel(const OptArgs g) {
    constexpr int WC = opt_wc<DIM>();
    __shared__ double wave_acc[4][WC][DIM * DIM * 2];
    const int tid = (int)threadIdx.x;
    const int n = g.n;
    const int64_t k = blockIdx.x;
    const int64_t pairs = (int64_t)n * n;
    const double* Ek = g.E + (size_t)k * n;
    const double *fk = g.tab + (size_t)k * n, *gk = fk + (size_t)g.nkc * n;
    const double2* Vk = g.D + (size_t)k * g.d_sk;
    const double2* Pk = g.P ? g.P + (size_t)k * g.d_sk : nullptr;
    const double eta = g.eta, eta2 = eta * eta;
    for (int w0 = 0; w0 < g.nw; w0 += WC) {
        double om[WC], acc[WC][DIM * DIM * 2];
#pragma unroll
        for (int j = 0; j < WC; ++j) {
            om[j] = g.W[w0 + j < g.nw ? w0 + j : g.nw - 1];
#pragma unroll
            for (int x = 0; x < DIM * DIM * 2; ++x) acc[j][x] = 0.0;
        }
        for (int64_t e = tid; e < pairs; e += OPT_THREADS) {
            const int b = (int)(e / n), c = (int)(e - (int64_t)b * n);
            const double de = Ek[b] - Ek[c];
            double er[DIM], ei[DIM];
#pragma unroll
            for (int a = 0; a < DIM; ++a) {
                const double2 v = Vk[(size_t)a * g.d_sa + e];
                er[a] = v.x;
                ei[a] = v.y;
                if (Pk) {
                    const double2 p = Pk[(size_t)a * g.d_sa + e];
                    er[a] = fma(-de, p.y, er[a]);
                    ei[a] = fma(de, p.x, ei[a]);
                }
            }
            const double t = chi_pair_weight(Ek[b], fk[b], gk[b], Ek[c], fk[c], gk[c], g.inv_t);
            opt_element<DIM, WC>(t, er, ei, de, om, eta, eta2, acc);
        }
        opt_store_chunk<DIM, WC, 1>(acc, wave_acc, g, k, true, w0, tid);
    }
}

// T[k][b][i] = pos[i][a] conj(U[k][i][b]): the library's right operand of U^H diag(pos_a) U (see opt_library_products)
__global__ void __launch_bounds__(OPT_THREADS) opt_scale_kernel(const double2* __restrict__ U, const double* __restrict__ pos, int n, int dim, int a,
                                                                int64_t total, double2* __restrict__ T) {
    const int64_t idx = (int64_t)blockIdx.x * OPT_THREADS + threadIdx.x;
    if (idx >= total) return;
    const int64_t nn = (int64_t)n * n, k = idx / nn, rem = idx - k * nn;
    const int b = (int)(rem / n), i = (int)(rem - (int64_t)b * n);
    const double2 u = U[(size_t)k * nn + (size_t)i * n + b];
    const double p = pos[(size_t)i * dim + a];
    T[idx] = make_double2(p * u.x, -(p * u.y));
}

// groups[g0 + g][omega][a][c] = the partials of the slab's points [256 g, 256 g + 256) in index order, per component: thread x one of
// the `row` = nw DIM DIM 2 doubles of a point.  grid: (row / 256, groups of the slab)
__global__ void __launch_bounds__(OPT_THREADS) opt_group_kernel(const double* __restrict__ part, int64_t nk, int64_t row, int64_t g0,
                                                                double* __restrict__ groups) {
    const int64_t x = (int64_t)blockIdx.x * OPT_THREADS + threadIdx.x;
    if (x >= row) return;
    const int64_t k0 = (int64_t)blockIdx.y * OPT_GROUP, k1 = k0 + OPT_GROUP < nk ? k0 + OPT_GROUP : nk;
    double sum = 0.0;
    for (int64_t k = k0; k < k1; ++k) sum += part[(size_t)k * row + x];
    groups[(size_t)(g0 + blockIdx.y) * row + x] = sum;
}

// sigma[w_first + omega][a][c] = i S / T / NK, S the groups in index order: thread e one of the nw DIM DIM complex numbers
__global__ void __launch_bounds__(OPT_THREADS) opt_final_kernel(const double2* __restrict__ groups, int64_t n_groups, int64_t entries, double T, double nk,
                                                                double2* __restrict__ sigma) {
    const int64_t e = (int64_t)blockIdx.x * OPT_THREADS + threadIdx.x;
    if (e >= entries) return;
    double sr = 0.0, si = 0.0;
    for (int64_t gi = 0; gi < n_groups; ++gi) {
        const double2 v = groups[(size_t)gi * entries + e];
        sr += v.x;
        si += v.y;
    }
    sigma[e] = make_double2((0.0 - si) / T / nk, (0.0 + sr) / T / nk);
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
struct OptPlan {
    int dim = 0, n = 0;
    int np = 0;           // the fused kernel's template (16, 32, 64), 0: the library route
    int wc = 0;           // frequencies per register chunk
    int64_t nk = 0;       // points of the mesh
    int64_t groups = 0;   // of 256 points
    int64_t n_w = 0, w_pass = 0, passes = 0;
    size_t per_w(int64_t points) const { return (size_t)points * dim * dim * sizeof(double2); }  // the partials of one frequency
    int64_t row(int64_t nw) const { return nw * dim * dim * 2; }                                 // doubles of one point's partials
};

// the one place that chooses: template, register chunk, the frequencies per pass from the bytes the partials of `points` mesh points
// may take (0: the budget)
void opt_plan_sizes(int64_t nk, int64_t points, int n_orb, int dim, int64_t n_w, size_t mem, OptPlan* L) {
    L->dim = dim;
    L->n = n_orb;
    L->np = n_orb <= 16 ? 16 : n_orb <= 32 ? 32 : n_orb <= OPT_FUSED_MAX ? 64 : 0;
    L->wc = dim == 2 ? opt_wc<2>() : opt_wc<3>();
    L->nk = nk;
    L->groups = (nk + OPT_GROUP - 1) / OPT_GROUP;
    L->n_w = n_w;
    const size_t room = mem == 0 ? OPT_PART_BUDGET : mem;
    const int64_t fit = (int64_t)std::min<size_t>(room / L->per_w(points), (size_t)1 << 62);
    L->w_pass = fit >= n_w ? n_w : fit >= L->wc ? fit / L->wc * L->wc : fit;
    L->passes = L->w_pass == 0 ? 0 : (n_w + L->w_pass - 1) / L->w_pass;
}

int opt_plan(int64_t nk, int64_t points, int n_orb, int dim, int64_t n_w, size_t mem, OptPlan* L) {
    opt_plan_sizes(nk, points, n_orb, dim, n_w, mem, L);
    if (L->w_pass < 1) {
        tbk_set_error("the partial sums of the optical conductivity at one frequency need %zu bytes of device memory", L->per_w(points));
        return TBK_ERR_MEMORY;
    }
    return TBK_OK;
}

int opt_check_frequencies(int64_t n_w, const double* omega, double eta) {
    return pair_check_frequencies(n_w, OPT_MAX_NW, omega, eta, "the optical conductivity takes up to 2^23 frequencies per call");
}

template <int NP, int DIM>
int opt_launch_fused_as(hipStream_t s, const OptArgs& a) {
    constexpr int KPW = NP == 16 ? 4 : 1;
    constexpr int lds = KPW * 4 * NP * NP * (int)sizeof(double);
    static tbk_flag_row raised;
    if (lds > 64 * 1024) TBK_HIP(tbk_raise_lds_limit(reinterpret_cast<const void*>(&opt_fused_kernel<NP, DIM>), lds, raised));
    hipLaunchKernelGGL((opt_fused_kernel<NP, DIM>), dim3((unsigned)((a.nkc + KPW - 1) / KPW)), dim3(OPT_THREADS), lds, s, a);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

template <int DIM>
int opt_launch_fused(hipStream_t s, int np, const OptArgs& a) {
    if (np == 16) return opt_launch_fused_as<16, DIM>(s, a);
    if (np == 32) return opt_launch_fused_as<32, DIM>(s, a);
    return opt_launch_fused_as<64, DIM>(s, a);
}

// what one chunk of the walk is made from, on either driver
struct OptChunk {
    hipStream_t s = nullptr;
    rocblas_handle blas = nullptr;  // the library route
    int64_t nkc = 0, k_off = 0;
    const double* d_E = nullptr;
    const double* d_U = nullptr;
    double* d_D = nullptr;          // D^a of point k at d_D + 2 (k d_sk + a d_sa); the library route overwrites it with V^a
    size_t d_sk = 0, d_sa = 0;      // in complex numbers
    const double* d_pos = nullptr;  // convention 1: [n][dim]
    double* d_tab = nullptr;        // [2][nkc n]
    double* d_T = nullptr;          // library: [nkc][n][n] complex
    double* d_P = nullptr;          // library, convention 1: U^H diag(pos_a) U with the strides of d_D
};

// The library route's products: V^a takes D^a's place (opt_library_rotate, tbk_velocity.h).  Convention 1: T = diag(pos_a) Uc^H from
// opt_scale_kernel, Pc = Uc T.  Calls stay below 2^29 elements, as those of tbk_eigh.
int opt_library_products(const OptPlan& L, const OptChunk& c) {
    const int n = L.n;
    const int64_t nn = (int64_t)n * n, step = std::max<int64_t>(1, (int64_t(1) << 29) / nn);
    const rocblas_double_complex one(1.0, 0.0), zero(0.0, 0.0);
    typedef rocblas_double_complex Z;
    for (int a = 0; a < L.dim; ++a)
        for (int64_t b0 = 0; b0 < c.nkc; b0 += step) {
            const rocblas_int nb = (rocblas_int)std::min(step, c.nkc - b0);
            const Z* Uc = reinterpret_cast<const Z*>(c.d_U) + (size_t)b0 * nn;
            Z* Da = reinterpret_cast<Z*>(c.d_D) + (size_t)b0 * c.d_sk + (size_t)a * c.d_sa;
            Z* Tc = reinterpret_cast<Z*>(c.d_T) + (size_t)b0 * nn;
            TBK_CHECK(opt_library_rotate(c.blas, n, nb, Uc, Da, c.d_sk, Tc));
            if (c.d_pos != nullptr) {
                Z* Pa = reinterpret_cast<Z*>(c.d_P) + (size_t)b0 * c.d_sk + (size_t)a * c.d_sa;
                const int64_t total = (int64_t)nb * nn;
                hipLaunchKernelGGL(opt_scale_kernel, dim3((unsigned)((total + OPT_THREADS - 1) / OPT_THREADS)), dim3(OPT_THREADS), 0, c.s,
                                   reinterpret_cast<const double2*>(Uc), c.d_pos, n, L.dim, a, total, reinterpret_cast<double2*>(Tc));
                TBK_HIP(hipGetLastError());
                TBK_ROCBLAS(rocblas_zgemm_strided_batched(c.blas, rocblas_operation_none, rocblas_operation_none, n, n, n, &one, Uc, n, (rocblas_stride)nn,
                                                          Tc, n, (rocblas_stride)nn, &zero, Pa, n, (rocblas_stride)c.d_sk, nb));
            }
        }
    return TBK_OK;
}

// stage 1 of a chunk: the Fermi tables, the rotation into the band basis and the epilogue of the pass's frequencies d_W[nw] into part
int opt_launch_chunk(const OptPlan& L, const OptChunk& c, SpanRecorder* ev, double mu, double T, const double* d_W, int64_t nw, double eta,
                     double* d_part) {
    const int64_t items = c.nkc * L.n;
    if (ev) ev->start(1);
    hipLaunchKernelGGL(chi_fermi_kernel, dim3((unsigned)((items + PAIR_THREADS - 1) / PAIR_THREADS)), dim3(PAIR_THREADS), 0, c.s, c.d_E, items, mu, T,
                       c.d_tab);
    TBK_HIP(hipGetLastError());
    OptArgs a;
    a.E = c.d_E;
    a.tab = c.d_tab;
    a.U = reinterpret_cast<const double2*>(c.d_U);
    a.D = reinterpret_cast<const double2*>(c.d_D);
    a.d_sk = c.d_sk;
    a.d_sa = c.d_sa;
    a.n = L.n;
    a.nkc = c.nkc;
    a.inv_t = 1.0 / T;
    a.W = d_W;
    a.nw = (int)nw;
    a.eta = eta;
    a.part = d_part;
    a.k_off = c.k_off;
    if (L.np != 0) {
        a.pos = c.d_pos;
        TBK_CHECK(L.dim == 2 ? opt_launch_fused<2>(c.s, L.np, a) : opt_launch_fused<3>(c.s, L.np, a));
    } else {
        TBK_CHECK(opt_library_products(L, c));
        if (c.d_pos != nullptr) a.P = reinterpret_cast<const double2*>(c.d_P);
        if (L.dim == 2)
            hipLaunchKernelGGL((opt_global_kernel<2>), dim3((unsigned)c.nkc), dim3(OPT_THREADS), 0, c.s, a);
        else
            hipLaunchKernelGGL((opt_global_kernel<3>), dim3((unsigned)c.nkc), dim3(OPT_THREADS), 0, c.s, a);
        TBK_HIP(hipGetLastError());
    }
    if (ev) ev->stop();
    return TBK_OK;
}

// stage 2 of a slab: its `points` partials into its groups, from g0 on in d_groups
int opt_launch_groups(hipStream_t s, const OptPlan& L, SpanRecorder* ev, const double* d_part, int64_t points, int64_t nw, int64_t g0, double* d_groups) {
    const int64_t row = L.row(nw), slab_groups = (points + OPT_GROUP - 1) / OPT_GROUP;
    if (ev) ev->start(2);
    hipLaunchKernelGGL(opt_group_kernel, dim3((unsigned)((row + OPT_THREADS - 1) / OPT_THREADS), (unsigned)slab_groups), dim3(OPT_THREADS), 0, s, d_part,
                       points, row, g0, d_groups);
    if (ev) ev->stop();
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

int opt_launch_final(hipStream_t s, const OptPlan& L, SpanRecorder* ev, const double* d_groups, int64_t nw, double T, double* d_sigma) {
    const int64_t entries = L.row(nw) / 2;
    if (ev) ev->start(2);
    hipLaunchKernelGGL(opt_final_kernel, dim3((unsigned)((entries + OPT_THREADS - 1) / OPT_THREADS)), dim3(OPT_THREADS), 0, s,
                       reinterpret_cast<const double2*>(d_groups), L.groups, entries, T, (double)L.nk, reinterpret_cast<double2*>(d_sigma));
    if (ev) ev->stop();
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

}  // namespace

extern "C" int tbk_optics_plan(int64_t nk, int n_orb, int dim, int64_t n_w, int64_t part_bytes, int64_t* out) {
    TBK_ARG(nk >= 1 && nk <= OPT_MAX_NK && n_orb >= 1 && (dim == 2 || dim == 3) && n_w >= 1 && n_w <= OPT_MAX_NW && part_bytes >= 0 && out != nullptr,
            "nk / n_orb / n_w < 1, more than 2^23 points or frequencies, dim not 2 or 3, part_bytes < 0 or out is NULL");
    OptPlan L;
    opt_plan_sizes(nk, nk, n_orb, dim, n_w, (size_t)part_bytes, &L);
    out[0] = L.np;
    out[1] = L.wc;
    out[2] = L.w_pass;
    out[3] = L.passes;
    out[4] = L.groups;
    return TBK_OK;
}

extern "C" int tbk_optics_from_eigensystem(int device, int dim, int n_orb, int64_t nk, const double* E, const double* U, const double* D,
                                           const double* pos, double mu, double T, int64_t n_w, const double* omega, double eta, int64_t part_bytes,
                                           double* sigma_out) {
    TBK_ARG(dim == 2 || dim == 3, "the optical conductivity needs a 2- or 3-dimensional model");
    TBK_ARG(n_orb >= 1 && nk >= 1 && nk <= OPT_MAX_NK, "n_orb / nk < 1 or more than 2^23 points");
    TBK_ARG(E != nullptr && U != nullptr && D != nullptr && sigma_out != nullptr, "E / U / D / sigma is NULL");
    TBK_ARG(std::isfinite(mu), "the chemical potential is not finite");
    TBK_ARG(std::isfinite(T) && T > 0.0, "the temperature is not finite or not positive");
    TBK_CHECK(opt_check_frequencies(n_w, omega, eta));
    TBK_ARG(part_bytes >= 0, "part_bytes < 0");
    TBK_CHECK(tetra_check_device(device));
    OptPlan L;
    TBK_CHECK(opt_plan(nk, nk, n_orb, dim, n_w, (size_t)part_bytes, &L));
    const size_t nn = (size_t)n_orb * n_orb, d2 = (size_t)dim * dim;
    const size_t e_bytes = (size_t)nk * n_orb * sizeof(double), u_bytes = (size_t)nk * nn * sizeof(double2);
    DevBuf d_E, d_U, d_D, d_pos, d_tab, d_T, d_P, d_W, d_part, d_groups, d_sigma;
    Owned<rocblas_handle, rocblas_destroy_handle> blas;
    TBK_CHECK(d_E.reserve(e_bytes));
    TBK_CHECK(d_tab.reserve(2 * e_bytes));
    TBK_CHECK(mesh_reserve(d_U, u_bytes, OPT_FAMILY, "the eigenvectors"));
    TBK_CHECK(mesh_reserve(d_D, u_bytes * dim, OPT_FAMILY, "the derivatives"));
    TBK_CHECK(d_W.reserve((size_t)n_w * sizeof(double)));
    TBK_CHECK(d_part.reserve((size_t)L.w_pass * L.per_w(nk)));
    TBK_CHECK(d_groups.reserve((size_t)L.groups * L.w_pass * d2 * sizeof(double2)));
    TBK_CHECK(d_sigma.reserve((size_t)n_w * d2 * sizeof(double2)));
    if (pos) {
        TBK_CHECK(d_pos.reserve((size_t)n_orb * dim * sizeof(double)));
        TBK_HIP(hipMemcpy(d_pos.ptr, pos, (size_t)n_orb * dim * sizeof(double), hipMemcpyHostToDevice));
    }
    if (L.np == 0) {
        TBK_CHECK(mesh_reserve(d_T, u_bytes, OPT_FAMILY, "the library's products"));
        if (pos) TBK_CHECK(mesh_reserve(d_P, u_bytes * dim, OPT_FAMILY, "the library's products"));
        TBK_ROCBLAS(rocblas_create_handle(blas.put()));
    }
    TBK_HIP(hipMemcpy(d_E.ptr, E, e_bytes, hipMemcpyHostToDevice));
    TBK_HIP(hipMemcpy(d_U.ptr, U, u_bytes, hipMemcpyHostToDevice));
    TBK_HIP(hipMemcpy(d_W.ptr, omega, (size_t)n_w * sizeof(double), hipMemcpyHostToDevice));
    OptChunk c;
    c.blas = blas;
    c.nkc = nk;
    c.d_E = d_E.as<double>();
    c.d_U = d_U.as<double>();
    c.d_D = d_D.as<double>();
    c.d_sk = nn * dim;
    c.d_sa = nn;
    c.d_pos = pos ? d_pos.as<double>() : nullptr;
    c.d_tab = d_tab.as<double>();
    c.d_T = d_T.as<double>();
    c.d_P = d_P.as<double>();
    for (int64_t w0 = 0; w0 < n_w; w0 += L.w_pass) {
        const int64_t nw = std::min(L.w_pass, n_w - w0);
        // (the library route overwrites D^a with V^a: every pass starts from the caller's)
        TBK_HIP(hipMemcpy(d_D.ptr, D, u_bytes * dim, hipMemcpyHostToDevice));
        TBK_CHECK(opt_launch_chunk(L, c, nullptr, mu, T, d_W.as<double>() + w0, nw, eta, d_part.as<double>()));
        TBK_CHECK(opt_launch_groups(nullptr, L, nullptr, d_part.as<double>(), nk, nw, 0, d_groups.as<double>()));
        TBK_CHECK(opt_launch_final(nullptr, L, nullptr, d_groups.as<double>(), nw, T, d_sigma.as<double>() + (size_t)w0 * d2 * 2));
    }
    TBK_HIP(hipMemcpy(sigma_out, d_sigma.ptr, (size_t)n_w * d2 * sizeof(double2), hipMemcpyDeviceToHost));
    return TBK_OK;
}

extern "C" int tbk_optical_conductivity_multi(tbk_model* const* handles, int n_handles, const int32_t* mesh, int mode, double value, double T,
                                              int64_t n_w, const double* omega, double eta, int convention, const double* pos, int64_t part_bytes,
                                              double* mu_out, double* sigma_out) {
    TBK_ARG(mu_out != nullptr && sigma_out != nullptr, "mu / sigma is NULL");
    TBK_ARG(mode == 0 || mode == 1, "mode must be 0 (value = energy) or 1 (value = n_electrons)");
    TBK_ARG(handles != nullptr && n_handles >= 1 && handles[0] != nullptr, "no handles");
    TBK_ARG(std::isfinite(T) && T > 0.0, "the temperature is not finite or not positive");
    TBK_CHECK(opt_check_frequencies(n_w, omega, eta));
    TBK_CHECK(tbk_eigh_check_arguments(0, convention, pos));
    TBK_ARG(part_bytes >= 0, "part_bytes < 0");
    if (mode == 1)
        TBK_CHECK(tbk_fermi_check_electrons(value, handles[0]->n_orb));
    else
        TBK_ARG(std::isfinite(value), "the energy is not finite");
    // mu: the slab route of tbk_occupations as it stands
    OccStaged staged;
    TBK_CHECK(staged.make(handles, n_handles, mesh));
    TBK_CHECK(staged.find_mu(mesh, mode, value, mu_out));
    const double mu = mu_out[0];
    const int n = staged.n_orb, dim = staged.dim;
    const int64_t nk = staged.nk_total;
    TBK_ARG(nk <= OPT_MAX_NK, "the optical conductivity takes meshes of up to 2^23 points");
    const size_t nn = (size_t)n * n, d2 = (size_t)dim * dim;
    // the handles take whole groups of 256 points: the sum is the same sum whatever their number
    const int64_t groups = (nk + OPT_GROUP - 1) / OPT_GROUP;
    const TetraSlabs cut(groups, n_handles);
    const int busy = cut.busy();
    // (h_k and h_groups are the sources and targets of enqueued copies: in front of `streams`, which waits before they go)
    std::vector<double> h_k;
    TBK_CHECK(tbk_dos_mesh_klist(dim, mesh, 0, mesh[0], &h_k));
    std::vector<std::vector<double>> h_groups((size_t)busy);
    MeshStreams streams;
    struct Slab {
        tbk_model* m;
        SpanRecorder* ev;
        int64_t k_lo, points, chunk;
        OptPlan L;
    };
    std::vector<Slab> slabs;
    const bool with_pos = convention == 1;
    // the reservations of every handle, then one plan for the passes: the fewest frequencies any handle's partials leave room for
    int64_t w_pass = n_w;
    for (int i = 0; i < busy; ++i) {
        tbk_model* m = handles[i];  // (locked by staged)
        TBK_CHECK(streams.add(m));
        Slab s;
        s.m = m;
        s.ev = &streams.used.back().ev;
        s.k_lo = cut.lo(i) * OPT_GROUP;
        s.points = std::min(nk, (cut.lo(i) + cut.count(i)) * OPT_GROUP) - s.k_lo;
        size_t free_b = 0, total_b = 0;
        TBK_HIP(hipMemGetInfo(&free_b, &total_b));
        const size_t room = part_bytes > 0 ? (size_t)part_bytes : std::max<size_t>(1, std::min(OPT_PART_BUDGET, std::max(m->ws_dm_part.bytes, free_b / 4)));
        TBK_CHECK(opt_plan(nk, s.points, n, dim, n_w, room, &s.L));
        w_pass = std::min(w_pass, s.L.w_pass);
        slabs.push_back(s);
    }
    const int64_t passes = (n_w + w_pass - 1) / w_pass;
    for (Slab& s : slabs) {
        tbk_model* m = s.m;
        TBK_HIP(hipSetDevice(m->device));
        const bool library = s.L.np == 0;
        TBK_CHECK(m->ws_mesh_k.reserve((size_t)s.points * dim * sizeof(double)));
        TBK_CHECK(mesh_reserve(m->ws_dm_part, (size_t)w_pass * s.L.per_w(s.points), OPT_FAMILY, "the partial sums of one pass"));
        TBK_CHECK(m->ws_dm_rho.reserve(((size_t)groups + 1) * w_pass * d2 * sizeof(double2)));
        TBK_CHECK(m->ws_mesh_io.reserve(dos_align256((size_t)n_w * sizeof(double)) + (size_t)n * dim * sizeof(double)));
        // the chunk of the eigenvector walk from what is left: beside U the dim derivatives (the library route: its products too)
        const int share = 1 + dim + (library ? 1 + (with_pos ? dim : 0) : 0);
        s.chunk = mesh_eigh_chunk(m, s.points, share);
        // where H(k) has one arithmetic up to some chunk length (tbk_hk_stable_chunk), stay below it: then no bit knows the chunk
        if (tbk_hk_stable_chunk(m) > 0) s.chunk = std::min(s.chunk, tbk_hk_stable_chunk(m));
        const size_t u_bytes = (size_t)s.chunk * nn * sizeof(double2), e_bytes = (size_t)s.chunk * n * sizeof(double);
        TBK_CHECK(mesh_reserve(m->ws_pdos_u, u_bytes + 3 * e_bytes, OPT_FAMILY, "the eigenvectors of one chunk"));
        TBK_CHECK(mesh_reserve(m->ws_dm_p, u_bytes * dim, OPT_FAMILY, "the derivatives of one chunk"));
        if (library) {
            TBK_CHECK(mesh_reserve(m->ws_mesh_work, u_bytes * (1 + (with_pos ? dim : 0)), OPT_FAMILY, "the library's products of one chunk"));
            m->counters[TBK_CNT_LIBRARY_CALLS] += 1;
        }
        double* d_W = m->ws_mesh_io.as<double>();
        double* d_pos = reinterpret_cast<double*>(m->ws_mesh_io.as<char>() + dos_align256((size_t)n_w * sizeof(double)));
        TBK_HIP(hipMemcpyAsync(m->ws_mesh_k.ptr, h_k.data() + (size_t)s.k_lo * dim, (size_t)s.points * dim * sizeof(double), hipMemcpyHostToDevice, m->stream));
        TBK_HIP(hipMemcpyAsync(d_W, omega, (size_t)n_w * sizeof(double), hipMemcpyHostToDevice, m->stream));
        if (with_pos) TBK_HIP(hipMemcpyAsync(d_pos, pos, (size_t)n * dim * sizeof(double), hipMemcpyHostToDevice, m->stream));
    }
    for (int64_t pass = 0; pass < passes; ++pass) {
        const int64_t w0 = pass * w_pass, nw = std::min(w_pass, n_w - w0);
        const size_t g_row = (size_t)nw * d2 * 2;  // doubles of one group
        for (size_t i = 0; i < slabs.size(); ++i) {
            Slab& s = slabs[i];
            tbk_model* m = s.m;
            TBK_HIP(hipSetDevice(m->device));
            const bool library = s.L.np == 0;
            const size_t u_doubles = (size_t)s.chunk * nn * 2;
            double* d_U = m->ws_pdos_u.as<double>();
            double* d_E = d_U + u_doubles;
            const double* d_k = m->ws_mesh_k.as<double>();
            const double* d_W = m->ws_mesh_io.as<double>();
            const double* d_pos = reinterpret_cast<const double*>(m->ws_mesh_io.as<char>() + dos_align256((size_t)n_w * sizeof(double)));
            for (int64_t c0 = 0; c0 < s.points; c0 += s.chunk) {
                const int64_t nkc = std::min(s.chunk, s.points - c0);
                TBK_CHECK(tbk_eigh_device_rows(m, d_k + c0 * dim, nkc, 2, nullptr, d_E, d_U, true));
                s.ev->start(0);
                int status = TBK_OK;
                for (int a = 0; a < dim && status == TBK_OK; ++a)
                    status = tbk_chunk_dh(m, a, d_k + c0 * dim, nkc, m->ws_dm_p.as<double>() + (size_t)a * nkc * nn * 2);
                s.ev->stop();  // (before the status is looked at: no span stays open)
                TBK_CHECK(status);
                OptChunk c;
                c.s = m->stream;
                c.blas = library ? (rocblas_handle)m->blas : nullptr;
                c.nkc = nkc;
                c.k_off = c0;
                c.d_E = d_E;
                c.d_U = d_U;
                c.d_D = m->ws_dm_p.as<double>();
                c.d_sk = nn;
                c.d_sa = (size_t)nkc * nn;
                c.d_pos = with_pos ? d_pos : nullptr;
                c.d_tab = d_E + (size_t)s.chunk * n;
                c.d_T = m->ws_mesh_work.as<double>();
                c.d_P = library && with_pos ? m->ws_mesh_work.as<double>() + (size_t)nkc * nn * 2 : nullptr;
                TBK_CHECK(opt_launch_chunk(s.L, c, s.ev, mu, T, d_W + w0, nw, eta, m->ws_dm_part.as<double>()));
            }
            // the slab's groups at their places in the mesh's list; the later handles' go to the first through the host
            TBK_CHECK(opt_launch_groups(m->stream, s.L, s.ev, m->ws_dm_part.as<double>(), s.points, nw, s.k_lo / OPT_GROUP, m->ws_dm_rho.as<double>()));
            if (i > 0) {
                const size_t count = (size_t)((s.points + OPT_GROUP - 1) / OPT_GROUP) * g_row;
                try {
                    h_groups[i].resize(count);
                } catch (...) {
                    tbk_set_error("cannot allocate the per-handle results");
                    return TBK_ERR_MEMORY;
                }
                TBK_HIP(hipMemcpyAsync(h_groups[i].data(), m->ws_dm_rho.as<double>() + (size_t)(s.k_lo / OPT_GROUP) * g_row, count * sizeof(double),
                                       hipMemcpyDeviceToHost, m->stream));
            }
        }
        if (slabs.size() > 1) TBK_CHECK(streams.check());  // (synchronises every handle; the eigensolver's flags are reported as by tbk_eigh)
        Slab& first = slabs[0];
        tbk_model* m = first.m;
        TBK_HIP(hipSetDevice(m->device));
        for (size_t i = 1; i < slabs.size(); ++i)
            TBK_HIP(hipMemcpyAsync(m->ws_dm_rho.as<double>() + (size_t)(slabs[i].k_lo / OPT_GROUP) * g_row, h_groups[i].data(),
                                   h_groups[i].size() * sizeof(double), hipMemcpyHostToDevice, m->stream));
        double* d_sigma = m->ws_dm_rho.as<double>() + (size_t)groups * w_pass * d2 * 2;
        TBK_CHECK(opt_launch_final(m->stream, first.L, first.ev, m->ws_dm_rho.as<double>(), nw, T, d_sigma));
        TBK_HIP(hipMemcpyAsync(sigma_out + (size_t)w0 * d2 * 2, d_sigma, g_row * sizeof(double), hipMemcpyDeviceToHost, m->stream));
        if (pass + 1 < passes) TBK_CHECK(streams.check());  // (the next pass overwrites the groups and the host buffers)
    }
    return streams.finish(TIMED_OPTICS);
}

extern "C" int tbk_optical_conductivity(tbk_model* m, const int32_t* mesh, int mode, double value, double T, int64_t n_w, const double* omega, double eta,
                                        int convention, const double* pos, int64_t part_bytes, double* mu_out, double* sigma_out) {
    return tbk_optical_conductivity_multi(&m, 1, mesh, mode, value, T, n_w, omega, eta, convention, pos, part_bytes, mu_out, sigma_out);
}

extern "C" int tbk_optics_timing(tbk_model* m, double* ms, int64_t* calls, int reset) {
    TBK_ARG(m != nullptr && ms != nullptr && calls != nullptr, "model / ms / calls is NULL");
    return tbk_timed_read(m, TIMED_OPTICS, 3, ms, calls, nullptr, reset);
}
