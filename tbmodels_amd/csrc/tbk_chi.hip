// tbk_chi.hip -- the bare (Lindhard) static susceptibility chi_0(q) of a uniform, periodic k mesh at one chemical potential and one
// temperature.  Not in the reference; DESIGN.md section 15 has the quantity, the kernels, the error bound and the measurements,
// tools/chi_model.py is the statement the tests compare with.
//
//   M(k, q)[b][b'] = sum_i conj(U[k][i][b]) D(q)[i] U[k+q][i][b']                U of tbk_eigh_device (convention 2), D: 1 or the
//   chi_0(q)       = -(1 / NK) sum_k sum_{b b'} F(E[k][b], E[k+q][b']) |M|^2     orbital phases of convention 1 (a host table)
//   F(a, b)        = (f(a) - f(b)) / (a - b) = -f(lo) (1 - f(hi)) h(y) / T       lo <= hi, y = (lo - hi) / T <= 0, h = expm1(y) / y
//
// k+q is the mesh point with the indices (i_d + q_d) mod n_d; the host reduces every q_d to [0, n_d) first, so q and q + n_d e_d
// are the same arguments of the kernels.  The eigensystem of the WHOLE mesh is resident (U: NK n^2 complex), every (k, q) pair reads
// two of its matrices.
//
//   chi_fermi_kernel    tab[0][k][b] = f(E), tab[1][k][b] = 1 - f(E) = f(2 mu - E), both from one exp(-|E - mu| / T): once per call.
//   chi_overlap_kernel  M = U(k)^H D U(k+q) as four real products on v_mfma_f64_16x16x4_f64, contraction over the orbitals:
//                       Mr = Ur^T U'r + Ui^T U'i, Mi = Ur^T U'i - Ui^T U'r (the minus is the instruction's negate-A bit).  A workgroup
//                       owns a 64 x 64 block of one M(k, q), wave t its tile row t (16 x 16 of four k-points up to 16 orbitals, a
//                       wave each): panels of 16 orbitals go through LDS once, orbital-major planes Ur, Ui (bands of the block's
//                       rows, of k) and Re, Im of D U' (bands of its columns, of k+q), padded with zeros to the tile.  U[k][i][.] is
//                       band-contiguous, so a panel row is one contiguous segment, and D is applied while staging: nothing but
//                       ds_read_b64 and MFMA inside the loop.  M is never stored: the epilogue forms |M|^2 f(lo) (1 - f(hi)) h(y)
//                       per accumulator element from the tables, the two eigenvalues and one expm1, masks the padding, and adds
//                       up in a fixed order -- the lane's elements, the wave's lanes, the block's waves -- to one double in
//                       part[q][k][block].
//   chi_pair_kernel     the same sum with |M|^2 = 1 (no eigenvectors): a wave per (k, q), the n^2 pairs in lane-strided order.
//   chi_reduce_kernel   chi[q] = (sum of part[q][.][.] in a fixed order) / T / NK: a workgroup per q, no atomics.
//
// The q list goes in batches of tbk_chi_plan's size (the memory of `part`).  For given (E, U, mu, T) the bits of chi_0(q) depend on
// q modulo the mesh and on D(q) alone: not on the batch, the other vectors, their order or the handle that computes them.
//
// The dynamic chi_0(q, omega_j + i eta) (chi_model.dynamic_susceptibility) takes the same overlaps and another
// epilogue:
//
//   chi_0(q, z) = -(1 / NK) sum_k sum_{b b'} g / (Delta + z) |M|^2       g = f(E[k][b]) - f(E[k+q][b']) = +-f(lo) (1 - f(hi)) (-expm1(y)),
//                                                                        Delta = E[k][b] - E[k+q][b'], + where E[k][b] <= E[k+q][b']
//
//   chi_overlap_kernel<BT, true>  keeps p = g |M|^2 and Delta of the lane's 4 BT elements in registers and walks the frequencies in
//                       chunks of CHI_WC per-lane (Re, Im) accumulators: x = Delta + omega, r = 1 / (x^2 + eta^2), t = p r,
//                       Re += t x, Im -= t eta, the lane's elements in register order, then the wave's lanes and the block's waves
//                       as above: one complex partial in part[q][omega][k][block].  Every frequency of a chunk runs the same
//                       instructions on its own accumulators (a short chunk is filled up with copies of its last frequency, which
//                       are not stored), so the bits of one (q, omega) do not know its place in the chunk, the pass or the list.
//   chi_pair_dyn_kernel the same with |M|^2 = 1, chi_pair_kernel's walk once per chunk.
//   chi_reduce_dyn_kernel  chi[q][omega] = (0 - sum of part[q][omega][.][.] in chi_reduce_kernel's order) / NK per component: the
//                       difference from +0 so that sums that are zeros of either sign give +0.
//
// Frequencies go in passes of tbk_chi_dynamic_plan's size when the partials of one vector for all of them do not fit; the overlaps
// are computed again per pass.
//
// The orbital-resolved chi_0[i][j](q) (chi_model.orbital_susceptibility) keeps the orbital indices that M sums
// away:
//
//   A(k, q)[i; b, b'] = conj(U[k][i][b]) D(q)[i] U[k+q][i][b']
//   chi_0[i][j](q)    = (1 / (T NK)) sum_k sum_{b b'} t A[i; b, b'] conj(A[j; b, b'])        t = f(lo) (1 - f(hi)) h(y) = -T F
//
//   chi_orbital_kernel<BT>  one Hermitian rank-K update per vector, K = (k, b, b'), on v_mfma_f64_16x16x4_f64: the operands X = t A and
//                       Y = A are made while staging, the block of (i, j) stays in registers over a slice of k-points, one complex
//                       partial block goes to part[q][slice][i][j].  Blocks with bi <= bj of the ascending selection only.
//   chi_reduce_orb_kernel  the slices in index order, / T / NK, the entry and its mirror (the conjugate) at the caller's places.
//
// tbk_chi_orbital_plan chooses template, slice length (a function of NK and n_orb alone), slices and batch.
//
// The orbital-resolved dynamic chi_0[i][j](q, omega + i eta) (chi_model.dynamic_orbital_susceptibility) puts the
// dynamic call's complex weight into the orbital call's update; the sum is not Hermitian, so every block and tile is computed and written:
//
//   chi_0[i][j](q, z) = -(1 / NK) sum_k sum_{b b'} g / (Delta + z) A[i; b, b'] conj(A[j; b, b'])      g, Delta as in the dynamic call
//
//   chi_orbital_dyn_kernel<BT, CHI_OWC>  one complex-weighted rank-K product X(omega) A^H per (vector, frequency), X = c A with
//                       c = (g r x, -(g r eta)), x = Delta + omega, r = 1 / (x^2 + eta^2): chi_orbital_kernel's geometry and walk, all
//                       nb^2 ordered blocks, frequencies in register chunks of CHI_OWC that share the staging of A, one complex partial
//                       block in part[q][omega][slice][i][j].
//   chi_reduce_orb_dyn_kernel  chi[q][omega][i][j] = (0 - the slices in index order) / NK per component, all m^2 entries.
//
// tbk_chi_orbital_dynamic_plan chooses template, blocks, slice length, slices, the vectors per batch and the frequency passes.
//
// The four-index chi_0[i][l][j][m](q) (chi_model.susceptibility_tensor; convention 2 only) keeps both orbital
// indices of each vertex and factorises per (k, b):
//
//   P[i][j] = conj(U[k][i][b]) U[k][j][b]         Q[l][m] = sum_b' t[b][b'] U[k+q][l][b'] conj(U[k+q][m][b'])
//   chi_0[i][l][j][m](q) = (1 / (T NK)) sum_k sum_b P[i][j] Q[l][m]
//
//   chi_tensor_kernel   a workgroup owns a 64 x 64 block of X[(i, j)][(l, m)] (rows: the pairs i <= j of the ascending selection, the
//                       others are conjugates) over a slice of k-points.  Per k and panel of 16 b: stage A, Q[(l, m)][b] = W t with
//                       W[(l, m)][b'] = U'[l][b'] conj(U'[m][b']) over panels of 16 b' (complex by real: two MFMAs per step), whose tile
//                       goes to LDS beside P; stage B, the plain transposed rank-16 update X += P Q^T (zmfma_ab) on the block in registers.
//   chi_reduce_ten_kernel  the slices in index order, / T / NK, the entry and its mirror at the caller's [i][l][j][m].
//
// tbk_chi_tensor_plan chooses blocks, slice length (a function of NK and n_orb alone), slices and batch.

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "tbk_occ.h"
#include "tbk_pair.h"
#include "tbk_zmfma.h"

namespace {

constexpr int CHI_THREADS = PAIR_THREADS;
constexpr int64_t CHI_MAX_BATCH = 4096;                 // vectors per launch (grid z), at most
constexpr size_t CHI_PART_BUDGET = size_t(256) << 20;   // the partials of one batch, at most
constexpr int64_t CHI_MAX_NK = int64_t(1) << 23;          // one grid column per k-point, 256 threads each
constexpr int CHI_MAX_ORB = 16320;                      // 255 x 255 blocks of one M: one grid row each
constexpr int CHI_WC = 8;                               // frequencies per chunk of the dynamic epilogue: 2 CHI_WC accumulators per lane
constexpr int64_t CHI_MAX_NW = int64_t(1) << 23;          // one grid column of the dynamic reduction per frequency, 256 threads each
constexpr int64_t CHI_GRID_YZ = 65535;                  // blocks along y or z of a grid, at most
constexpr int64_t CHI_ORB_MAX_NW = CHI_GRID_YZ;         // orbital-resolved dynamic: one grid row of its reduction per frequency of a pass

struct ChiMesh {
    int n[3];    // (n[2] = 1 in two dimensions)
    int64_t nk;  // points of the mesh
};

// the plan of a call of one of the five kinds: static (n_w = 0, m = 0), dynamic (n_w > 0), orbital-resolved (m > 0), orbital-resolved
// dynamic (m > 0 and n_w > 0), four-index (tr > 0)
struct ChiPlan {
    ChiMesh mesh;
    int n = 0;            // orbitals
    int bt = 0;           // template of the overlap kernel: 4, 1 (up to 16 orbitals), 0: no matrix elements (chi_pair_kernel);
                          // orbital-resolved: of chi_orbital_kernel, 4, 1 (m <= 16)
    int64_t blocks = 1;   // partials per (k, q); orbital-resolved: blocks with bi <= bj of one vector (dynamic: all nb^2 ordered blocks)
    int64_t batch = 1;    // vectors per launch
    int64_t batches = 1;
    int64_t n_w = 0;      // dynamic: frequencies
    int64_t w_pass = 0;   // ... per launch
    int64_t passes = 1;
    int m = 0;            // orbital-resolved: selected orbitals
    int mp = 0;           // ... padded to the block
    int64_t ks = 1;       // ... k-points per slice
    int64_t slices = 1;
    int64_t tr = 0;       // four-index: rows (pairs i <= j) and columns (pairs (l, m)) of one vector's partial matrix, padded to the
    int64_t tc = 0;       // block (0: not a four-index call)
    // the partials of one vector (dynamic: at one frequency), and of one batch
    size_t per_q() const {
        if (tr > 0) return (size_t)slices * (size_t)tr * (size_t)tc * sizeof(double2);
        return m > 0 ? (size_t)slices * mp * mp * sizeof(double2) : (size_t)mesh.nk * (size_t)blocks * (n_w == 0 ? sizeof(double) : sizeof(double2));
    }
    size_t part_bytes() const { return (size_t)batch * (n_w == 0 ? 1 : (size_t)w_pass) * per_q(); }
};

// what the dynamic epilogue reads besides the static one's arguments (all zero: the static kernels)
struct ChiDyn {
    const double* W = nullptr;  // the frequencies of this launch [nw], device memory
    int nw = 0;
    double eta = 0.0;
    double2* part = nullptr;    // [vectors of the batch][nw][NK][blocks]
};

// the one place that chooses: template, partials per pair, batch size from the bytes the partials may take (0: the budget)
void chi_plan_sizes(int64_t nk, int n_orb, int64_t n_q, bool matrix_elements, size_t mem, int* bt, int64_t* blocks, int64_t* batch,
                    int64_t* batches) {
    const int64_t nb = (n_orb + 63) / 64;
    *bt = !matrix_elements ? 0 : n_orb <= 16 ? 1 : 4;
    *blocks = *bt == 4 ? nb * nb : 1;
    const size_t per_q = (size_t)nk * (size_t)*blocks * sizeof(double);
    const size_t room = mem == 0 ? CHI_PART_BUDGET : mem;
    *batch = std::max<int64_t>(0, std::min<int64_t>(std::min(n_q, CHI_MAX_BATCH), (int64_t)(room / per_q)));
    *batches = *batch == 0 ? 0 : (n_q + *batch - 1) / *batch;
}

// the dynamic call's: as above, with 16 NK blocks bytes per (q, omega).  All frequencies of a vector in one launch when they fit (then
// as many vectors per batch as fit), else one vector per batch and the frequencies in passes (whole chunks of CHI_WC when one fits)
void chi_dyn_plan_sizes(int64_t nk, int n_orb, int64_t n_q, int64_t n_w, bool matrix_elements, size_t mem, int* bt, int64_t* blocks,
                        int64_t* batch, int64_t* batches, int64_t* w_pass, int64_t* passes) {
    const int64_t nb = (n_orb + 63) / 64;
    *bt = !matrix_elements ? 0 : n_orb <= 16 ? 1 : 4;
    *blocks = *bt == 4 ? nb * nb : 1;
    const size_t per_qw = (size_t)nk * (size_t)*blocks * sizeof(double2);
    const size_t room = mem == 0 ? CHI_PART_BUDGET : mem;
    const int64_t fit = (int64_t)std::min<size_t>(room / per_qw, (size_t)1 << 62);  // (q, omega) pairs whose partials fit
    if (fit >= n_w) {
        *w_pass = n_w;
        *batch = std::min<int64_t>(std::min(n_q, CHI_MAX_BATCH), fit / n_w);
    } else {
        *w_pass = fit >= CHI_WC ? fit / CHI_WC * CHI_WC : fit;
        *batch = fit >= 1 ? 1 : 0;
    }
    *passes = *w_pass == 0 ? 0 : (n_w + *w_pass - 1) / *w_pass;
    *batches = *batch == 0 ? 0 : (n_q + *batch - 1) / *batch;
}

// the flat index of k+q (q reduced to [0, n_d) per axis, three entries)
__device__ __forceinline__ int64_t chi_shifted(const ChiMesh& g, int64_t k, const int32_t* __restrict__ qv) {
    const int64_t i2 = k % g.n[2], r = k / g.n[2];
    const int64_t i1 = r % g.n[1], i0 = r / g.n[1];
    const int64_t j0 = (i0 + qv[0]) % g.n[0], j1 = (i1 + qv[1]) % g.n[1], j2 = (i2 + qv[2]) % g.n[2];
    return (j0 * g.n[1] + j1) * g.n[2] + j2;
}

// one pair of states at one frequency: re += t x, im -= t eta with t = p / (x^2 + eta^2), the multiply-adds fused as written
__device__ __forceinline__ void chi_dyn_term(double p, double delta, double omega, double eta, double eta2, double& re, double& im) {
    const double x = delta + omega;
    const double r = 1.0 / fma(x, x, eta2);
    const double t = p * r;
    re = fma(t, x, re);
    im = fma(-t, eta, im);
}

// BT tiles of 16 along each side of the workgroup's block of M: 4 (one k-point per workgroup, wave t owns tile row t) or 1 (n <= 16:
// four k-points per workgroup, one per wave).  grid: (k-points / KPW, blocks, vectors of the batch).  D: NULL or [batch][n] complex.
// DYN: the dynamic epilogue (dyn, not part, is written).
template <int BT, bool DYN>
__global__ void __launch_bounds__(CHI_THREADS) chi_overlap_kernel(const double2* __restrict__ U, const double* __restrict__ E,
                                                                  const double* __restrict__ tab, ChiMesh g, int n,
                                                                  const int32_t* __restrict__ Q, const double2* __restrict__ D, double inv_t,
                                                                  int64_t blocks, double* __restrict__ part, ChiDyn dyn) {
    using Geo = ZPanel<BT>;  // (tbk_zmfma.h; an item is a k-point)
    constexpr int RB = Geo::RB, KPW = Geo::KPW, TEAM = Geo::TEAM, S = Geo::S;
    static_assert(CHI_THREADS == Geo::THREADS, "the panel's workgroup");
    __shared__ double planes[KPW][4 * 16 * S];  // per k-point four planes [16][S]: Ur, Ui of the block's rows (k); Re, Im of D U' of its columns (k+q)
    __shared__ double wave_part[4];
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int team = BT == 1 ? wave : 0, tt = tid - team * TEAM;
    const int nb = (n + RB - 1) / RB;
    const int bi = (int)blockIdx.y / nb, bj = (int)blockIdx.y - bi * nb;
    const int64_t k = (int64_t)blockIdx.x * KPW + team;
    const int64_t ql = blockIdx.z;
    const bool valid = k < g.nk;
    const int64_t kp = valid ? chi_shifted(g, k, Q + ql * 3) : 0;
    const double2* Uk = U + (valid ? (size_t)k * n * n : 0);
    const double2* Up = U + (size_t)kp * n * n;
    const double2* Dq = D ? D + (size_t)ql * n : nullptr;
    const int ti = BT == 1 ? 0 : wave;                      // the wave's tile row
    const bool row_live = valid && bi * RB + ti * 16 < n;   // (wave-uniform)
    zd4 accr[BT], acci[BT];
    zpanel_overlap<BT>(Uk, Up, Dq, valid, n, n, bi, bj, planes[team], tt, ti, lane, row_live, accr, acci);  // M = U(k)^H D U(k+q)
    // the epilogue.  lane (q, c), register r: row q + 4 r, column c of the tile
    if constexpr (DYN) {
        __shared__ double wave_dyn[4][CHI_WC][2];
        // p = g |M|^2 (0 in the padding) of the lane's elements, once for all frequencies, and the eigenvalues of their rows and columns:
        // Delta = ea - eb is one subtraction per element and chunk, and half the registers of a stored one
        double pw[4 * BT], ea[4], ebv[BT];
#pragma unroll
        for (int e = 0; e < 4 * BT; ++e) pw[e] = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) ea[r] = 0.0;
#pragma unroll
        for (int tj = 0; tj < BT; ++tj) ebv[tj] = 0.0;
        if (row_live) {
            const int64_t items = g.nk * n;
            const double* Ea = E + (size_t)k * n;
            const double* Eb = E + (size_t)kp * n;
            const double *fa = tab + (size_t)k * n, *ga = fa + items, *fb = tab + (size_t)kp * n, *gb = fb + items;
            double fav[4], gav[4];
            bool a_in[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int b = bi * RB + ti * 16 + (lane >> 4) + 4 * r;
                a_in[r] = b < n;
                const int bs = a_in[r] ? b : 0;
                ea[r] = Ea[bs];
                fav[r] = fa[bs];
                gav[r] = ga[bs];
            }
#pragma unroll
            for (int tj = 0; tj < BT; ++tj) {
                const int c = bj * RB + tj * 16 + (lane & 15);
                if (bj * RB + tj * 16 < n) {  // (uniform)
                    const bool c_in = c < n;
                    const int cs = c_in ? c : 0;
                    const double eb = Eb[cs], fbv = fb[cs], gbv = gb[cs];
                    ebv[tj] = eb;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const double m2 = accr[tj][r] * accr[tj][r] + acci[tj][r] * acci[tj][r];
                        const double gd = chi_pair_difference(ea[r], fav[r], gav[r], eb, fbv, gbv, inv_t);
                        pw[tj * 4 + r] = (a_in[r] && c_in) ? gd * m2 : 0.0;
                    }
                }
            }
        }
        const double eta = dyn.eta, eta2 = eta * eta;
        for (int w0 = 0; w0 < dyn.nw; w0 += CHI_WC) {
            double om[CHI_WC], re[CHI_WC], im[CHI_WC];
#pragma unroll
            for (int j = 0; j < CHI_WC; ++j) {
                om[j] = dyn.W[w0 + j < dyn.nw ? w0 + j : dyn.nw - 1];  // (uniform; beyond the list: computed, not stored)
                re[j] = im[j] = 0.0;
            }
            if (row_live) {
#pragma unroll
                for (int tj = 0; tj < BT; ++tj) {
                    if (bj * RB + tj * 16 < n) {  // (uniform)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const double delta = ea[r] - ebv[tj];
#pragma unroll
                            for (int j = 0; j < CHI_WC; ++j) chi_dyn_term(pw[tj * 4 + r], delta, om[j], eta, eta2, re[j], im[j]);
                        }
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < CHI_WC; ++j) {
                re[j] = chi_wave_sum(re[j]);
                im[j] = chi_wave_sum(im[j]);
            }
            if (BT == 1) {
                if (valid && lane == 0) {
#pragma unroll
                    for (int j = 0; j < CHI_WC; ++j)
                        if (w0 + j < dyn.nw) dyn.part[((size_t)ql * dyn.nw + (w0 + j)) * g.nk + k] = make_double2(re[j], im[j]);
                }
            } else {
                if (lane == 0) {
#pragma unroll
                    for (int j = 0; j < CHI_WC; ++j) {
                        wave_dyn[wave][j][0] = re[j];
                        wave_dyn[wave][j][1] = im[j];
                    }
                }
                __syncthreads();
                if (tid < 2 * CHI_WC) {
                    const int j = tid >> 1, c = tid & 1;
                    if (w0 + j < dyn.nw)
                        reinterpret_cast<double*>(dyn.part)[((((size_t)ql * dyn.nw + (w0 + j)) * g.nk + k) * blocks + blockIdx.y) * 2 + c] =
                            ((wave_dyn[0][j][c] + wave_dyn[1][j][c]) + wave_dyn[2][j][c]) + wave_dyn[3][j][c];
                }
                __syncthreads();  // (the next chunk writes wave_dyn)
            }
        }
        return;
    }
    double sum = 0.0;
    if (row_live) {
        const int64_t items = g.nk * n;
        const double* Ea = E + (size_t)k * n;
        const double* Eb = E + (size_t)kp * n;
        const double *fa = tab + (size_t)k * n, *ga = fa + items, *fb = tab + (size_t)kp * n, *gb = fb + items;
        double ea[4], fav[4], gav[4];
        bool a_in[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int b = bi * RB + ti * 16 + (lane >> 4) + 4 * r;
            a_in[r] = b < n;
            const int bs = a_in[r] ? b : 0;
            ea[r] = Ea[bs];
            fav[r] = fa[bs];
            gav[r] = ga[bs];
        }
#pragma unroll
        for (int tj = 0; tj < BT; ++tj) {
            const int c = bj * RB + tj * 16 + (lane & 15);
            if (bj * RB + tj * 16 < n) {  // (uniform)
                const bool c_in = c < n;
                const int cs = c_in ? c : 0;
                const double eb = Eb[cs], fbv = fb[cs], gbv = gb[cs];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double m2 = accr[tj][r] * accr[tj][r] + acci[tj][r] * acci[tj][r];
                    const double w = chi_pair_weight(ea[r], fav[r], gav[r], eb, fbv, gbv, inv_t);
                    sum += (a_in[r] && c_in) ? w * m2 : 0.0;
                }
            }
        }
    }
    sum = chi_wave_sum(sum);
    if (BT == 1) {
        if (valid && lane == 0) part[(size_t)ql * g.nk + k] = sum;
    } else {
        if (lane == 0) wave_part[wave] = sum;
        __syncthreads();
        if (tid == 0) part[((size_t)ql * g.nk + k) * blocks + blockIdx.y] = ((wave_part[0] + wave_part[1]) + wave_part[2]) + wave_part[3];
    }
}

// |M|^2 = 1: a wave per (k, q), the n^2 pairs of states in lane-strided order.  grid: (k-points / 4, 1, vectors of the batch)
__global__ void __launch_bounds__(CHI_THREADS) chi_pair_kernel(const double* __restrict__ E, const double* __restrict__ tab, ChiMesh g, int n,
                                                               const int32_t* __restrict__ Q, double inv_t, double* __restrict__ part) {
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int64_t k = (int64_t)blockIdx.x * 4 + wave;
    const int64_t ql = blockIdx.z;
    const bool valid = k < g.nk;
    double sum = 0.0;
    if (valid) {
        const int64_t kp = chi_shifted(g, k, Q + ql * 3);
        const int64_t items = g.nk * n;
        const double *Ea = E + (size_t)k * n, *Eb = E + (size_t)kp * n;
        const double *fa = tab + (size_t)k * n, *ga = fa + items, *fb = tab + (size_t)kp * n, *gb = fb + items;
        const int64_t pairs = (int64_t)n * n;
        for (int64_t p = lane; p < pairs; p += 64) {
            const int a = (int)(p / n), b = (int)(p - (int64_t)a * n);
            sum += chi_pair_weight(Ea[a], fa[a], ga[a], Eb[b], fb[b], gb[b], inv_t);
        }
    }
    sum = chi_wave_sum(sum);
    if (valid && lane == 0) part[(size_t)ql * g.nk + k] = sum;
}

// chi[q] = (the len partials of q: thread t its contiguous piece in index order, then the threads in a fixed tree) / T / NK
__global__ void __launch_bounds__(CHI_THREADS) chi_reduce_kernel(const double* __restrict__ part, int64_t len, double T, double nk,
                                                                 double* __restrict__ chi) {
    __shared__ double red[CHI_THREADS];
    const int tid = (int)threadIdx.x;
    const double* p = part + (size_t)blockIdx.x * len;
    const int64_t piece = (len + CHI_THREADS - 1) / CHI_THREADS;
    const int64_t lo = tid * piece < len ? tid * piece : len, hi = lo + piece < len ? lo + piece : len;
    double acc = 0.0;
    for (int64_t i = lo; i < hi; ++i) acc += p[i];
    red[tid] = acc;
    __syncthreads();
    for (int s = CHI_THREADS / 2; s >= 1; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) chi[blockIdx.x] = red[0] / T / nk;
}

// chi_pair_kernel with the dynamic terms: the walk over the n^2 pairs once per chunk of frequencies.  part: [batch][nw][NK]
__global__ void __launch_bounds__(CHI_THREADS) chi_pair_dyn_kernel(const double* __restrict__ E, const double* __restrict__ tab, ChiMesh g, int n,
                                                                   const int32_t* __restrict__ Q, double inv_t, ChiDyn dyn) {
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int64_t k = (int64_t)blockIdx.x * 4 + wave;
    const int64_t ql = blockIdx.z;
    const bool valid = k < g.nk;
    const int64_t kp = valid ? chi_shifted(g, k, Q + ql * 3) : 0;
    const int64_t items = g.nk * n;
    const double *Ea = E + (size_t)(valid ? k : 0) * n, *Eb = E + (size_t)kp * n;
    const double *fa = tab + (size_t)(valid ? k : 0) * n, *ga = fa + items, *fb = tab + (size_t)kp * n, *gb = fb + items;
    const int64_t pairs = (int64_t)n * n;
    const double eta = dyn.eta, eta2 = eta * eta;
    for (int w0 = 0; w0 < dyn.nw; w0 += CHI_WC) {
        double om[CHI_WC], re[CHI_WC], im[CHI_WC];
#pragma unroll
        for (int j = 0; j < CHI_WC; ++j) {
            om[j] = dyn.W[w0 + j < dyn.nw ? w0 + j : dyn.nw - 1];
            re[j] = im[j] = 0.0;
        }
        if (valid) {
            for (int64_t p = lane; p < pairs; p += 64) {
                const int a = (int)(p / n), b = (int)(p - (int64_t)a * n);
                const double gd = chi_pair_difference(Ea[a], fa[a], ga[a], Eb[b], fb[b], gb[b], inv_t);
                const double delta = Ea[a] - Eb[b];
#pragma unroll
                for (int j = 0; j < CHI_WC; ++j) chi_dyn_term(gd, delta, om[j], eta, eta2, re[j], im[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < CHI_WC; ++j) {
            re[j] = chi_wave_sum(re[j]);
            im[j] = chi_wave_sum(im[j]);
        }
        if (valid && lane == 0) {
#pragma unroll
            for (int j = 0; j < CHI_WC; ++j)
                if (w0 + j < dyn.nw) dyn.part[((size_t)ql * dyn.nw + (w0 + j)) * g.nk + k] = make_double2(re[j], im[j]);
        }
    }
}

// chi[q][w_first + omega] = (0 - the len complex partials of (q, omega) in chi_reduce_kernel's order) / NK.  grid: (frequencies of the
// pass, vectors of the batch); chi: the batch's rows of [n_q][n_w]
__global__ void __launch_bounds__(CHI_THREADS) chi_reduce_dyn_kernel(const double2* __restrict__ part, int64_t len, double nk, int64_t n_w,
                                                                     int64_t w_first, double2* __restrict__ chi) {
    __shared__ double red[2][CHI_THREADS];
    const int tid = (int)threadIdx.x;
    const double2* p = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * len;
    const int64_t piece = (len + CHI_THREADS - 1) / CHI_THREADS;
    const int64_t lo = tid * piece < len ? tid * piece : len, hi = lo + piece < len ? lo + piece : len;
    double re = 0.0, im = 0.0;
    for (int64_t i = lo; i < hi; ++i) {
        const double2 v = p[i];
        re += v.x;
        im += v.y;
    }
    red[0][tid] = re;
    red[1][tid] = im;
    __syncthreads();
    for (int s = CHI_THREADS / 2; s >= 1; s >>= 1) {
        if (tid < s) {
            red[0][tid] += red[0][tid + s];
            red[1][tid] += red[1][tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) chi[(size_t)blockIdx.y * n_w + w_first + blockIdx.x] = make_double2((0.0 - red[0][0]) / nk, (0.0 - red[1][0]) / nk);
}

// ---- the orbital-resolved chi_0[i][j](q) ---------------------------------------------------------------------
// (a b) of two complex numbers, the multiply-adds fused as written: both templates of chi_orbital_kernel round alike
__device__ __forceinline__ double2 chi_cmul(double2 a, double2 b) {
    return make_double2(fma(a.x, b.x, -(a.y * b.y)), fma(a.x, b.y, a.y * b.x));
}

// The MFMAs of one staged panel of 16 b' on the wave's tile row ti and all BT tiles of the block: four steps of four b', the X pair
// read once per step, per tile the Y pair and the four real products of zmfma_abh.  No tile is guarded:
// a branch around an MFMA makes its accumulator a phi of two values, which the compiler keeps in VGPRs and copies to and from the
// AGPRs around every group of MFMAs (32 v_accvgpr moves and a drain of the pipe per four).  So the loop holds ds_read_b64 and MFMA
// only, and a tile that is never written (padding: zeros; below the diagonal of a diagonal block) is multiplied like any other.
template <int S, int BT>
__device__ __forceinline__ void chi_orb_tiles(const double (*pl)[16][S], int ti, int lane, zd4 (&accr)[BT], zd4 (&acci)[BT]) {
#pragma unroll 1
    for (int q4 = 0; q4 < 4; ++q4) {  // (not unrolled: ZPanel's note on registers)
        const int kq = 4 * q4 + (lane >> 4);
        const double xr = pl[0][kq][ti * 16 + (lane & 15)], xi = pl[1][kq][ti * 16 + (lane & 15)];
#pragma unroll
        for (int tj = 0; tj < BT; ++tj) {
            const double yr = pl[2][kq][tj * 16 + (lane & 15)], yi = pl[3][kq][tj * 16 + (lane & 15)];
            zmfma_abh(xr, xi, yr, yi, accr[tj], acci[tj]);
        }
    }
}

// One Hermitian rank-K update per vector, K = (k, b, b') of a slice of k-points: chi(q) = sum X Y^H with Y = A, X = t A,
// A[i; b, b'] = conj(U[k][i][b]) D[i] U[k+q][i][b'], t = chi_pair_weight(E[k][b], E[k+q][b']).  BT tiles of 16 along each side of the
// workgroup's block of (i, j): 4 (one slice per workgroup, wave t owns tile row t) or 1 (m <= 16: four slices per workgroup, one per
// wave).  grid: (slices / KPW, blocks with bi <= bj, vectors of the batch).  orb: the selected orbitals [m], ascending; rows of the
// padding are zeros.  Every element walks K in one order in both templates: k ascending, b ascending, b' ascending in panels of 16
// from 0, four b' per MFMA step -- and nothing else enters its bits.  The accumulators stay in registers over the whole slice; one
// complex partial block goes to part[q][slice][mp][mp] (tiles below the diagonal or of the
// padding are not written; <4> multiplies them all the same, see chi_orb_tiles).
template <int BT>
__global__ void __launch_bounds__(CHI_THREADS) chi_orbital_kernel(const double2* __restrict__ U, const double* __restrict__ E,
                                                                  const double* __restrict__ tab, ChiMesh g, int n,
                                                                  const int32_t* __restrict__ Q, const double2* __restrict__ D, double inv_t,
                                                                  const int32_t* __restrict__ orb, int m, int mp, int64_t ks, int64_t slices,
                                                                  double2* __restrict__ part) {
    using Geo = ZPanel<BT>;  // (tbk_zmfma.h; an item is a slice)
    constexpr int RB = Geo::RB, KPW = Geo::KPW, TEAM = Geo::TEAM, S = Geo::S;
    static_assert(CHI_THREADS == Geo::THREADS, "the panel's workgroup");
    constexpr int STEP = TEAM / 16;           // rows between the four a thread stages
    __shared__ double planes[KPW][4][16][S];  // Xr, Xi of the block's rows i; Yr, Yi of its columns j
    __shared__ double tw[KPW][TEAM];          // t[b][b'] of TEAM b' at once: one chi_pair_weight per (k, b, b')
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int team = BT == 1 ? wave : 0, tt = tid - team * TEAM;
    const int nb = mp / RB;
    int bi = 0, bj = (int)blockIdx.y;
    while (bj >= nb - bi) {
        bj -= nb - bi;
        ++bi;
    }
    bj += bi;
    const int64_t sl = (int64_t)blockIdx.x * KPW + team;
    const int64_t ql = blockIdx.z;
    const bool live = sl < slices;
    const int64_t k0 = live ? sl * ks : 0, k1 = live ? (k0 + ks < g.nk ? k0 + ks : g.nk) : 0;
    const double2* Dq = D ? D + (size_t)ql * n : nullptr;
    double(*pl)[16][S] = planes[team];
    double* twt = tw[team];
    const int ti = BT == 1 ? 0 : wave;               // the wave's tile row
    const bool row_live = bi * RB + ti * 16 < m;     // (wave-uniform)
    const bool diag = bi == bj;
    zd4 accr[BT], acci[BT];
#pragma unroll
    for (int tj = 0; tj < BT; ++tj) accr[tj] = acci[tj] = zd4{0.0, 0.0, 0.0, 0.0};
    // The accumulators' home is the AGPRs over all the loops below: an empty statement (no instruction) that reads them as AGPRs
    // stands behind the loops, and in <1> another ahead of them.  Without these the compiler keeps them in VGPRs and moves them in
    // and out around every group of MFMAs; where the statements must stand was read off the built code of each template
    // (DESIGN.md 17.2), and the no-copy state of both loops is what to look for after a compiler change.
    if constexpr (BT == 1) asm volatile("" : "+a"(accr[0]), "+a"(acci[0]));
    const int sb = tt & 15, srow0 = tt >> 4;  // the b' (row of the panel) and the first orbital row this thread stages
    int oi[4], oj[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int pi = bi * RB + srow0 + r * STEP, pj = bj * RB + srow0 + r * STEP;
        oi[r] = pi < m ? orb[pi] : -1;
        oj[r] = pj < m ? orb[pj] : -1;
    }
    const int64_t items = g.nk * n;
    const int64_t kn = BT == 1 ? ks : k1 - k0;  // (<1>: a team past its slice keeps the barriers; <4>: one slice, its own length)
    for (int64_t kk = 0; kk < kn; ++kk) {
        const int64_t k = k0 + kk;
        const bool valid = BT != 1 || k < k1;  // (uniform in the team)
        const int64_t kp = valid ? chi_shifted(g, k, Q + ql * 3) : 0;
        const double2* Uk = U + (valid ? (size_t)k * n * n : 0);
        const double2* Up = U + (size_t)kp * n * n;
        const double *Ea = E + (valid ? (size_t)k * n : 0), *Eb = E + (size_t)kp * n;
        const double *fa = tab + (valid ? (size_t)k * n : 0), *ga = fa + items, *fb = tab + (size_t)kp * n, *gb = fb + items;
        // <4>: the thread's entries of U[k+q] for a panel are loaded one panel ahead, under the MFMAs of the panel before (they do
        // not depend on b: the panel behind the last of one b is the first of the next); <1> loads them where it uses them and keeps
        // three waves per SIMD
        double2 ui[4], uj[4];
        auto fetch = [&](int p0) {
            const int bp = p0 + sb;
            const bool in = valid && bp < n;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                ui[r] = uj[r] = make_double2(0.0, 0.0);
                if (in && oi[r] >= 0) ui[r] = Up[(size_t)oi[r] * n + bp];
                if (!diag && in && oj[r] >= 0) uj[r] = Up[(size_t)oj[r] * n + bp];
            }
        };
        if constexpr (BT != 1) fetch(0);
        for (int b = 0; b < n; ++b) {
            // c = conj(U[k][i][b]) D[i] of the thread's rows: one value per i and b
            double2 ci[4], cj[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                ci[r] = cj[r] = make_double2(0.0, 0.0);
                if (valid && oi[r] >= 0) {
                    const double2 u = Uk[(size_t)oi[r] * n + b];
                    ci[r] = make_double2(u.x, -u.y);
                    if (Dq) ci[r] = chi_cmul(ci[r], Dq[oi[r]]);
                }
                if (!diag && valid && oj[r] >= 0) {
                    const double2 u = Uk[(size_t)oj[r] * n + b];
                    cj[r] = make_double2(u.x, -u.y);
                    if (Dq) cj[r] = chi_cmul(cj[r], Dq[oj[r]]);
                }
            }
            const double ea = Ea[b], fav = fa[b], gav = ga[b];
            for (int s0 = 0; s0 < n; s0 += TEAM) {
                {
                    // (the panels that read the previous weights are behind their second barrier)
                    const int bp = s0 + tt;
                    twt[tt] = (valid && bp < n) ? chi_pair_weight(ea, fav, gav, Eb[bp], fb[bp], gb[bp], inv_t) : 0.0;
                }
                const int s1 = s0 + TEAM < n ? s0 + TEAM : n;
                for (int p0 = s0; p0 < s1; p0 += 16) {
                    __syncthreads();  // the previous panel has been read, the weights are written
                    const int bp = p0 + sb;
                    const bool in = valid && bp < n;
                    const double t = twt[bp - s0];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = srow0 + r * STEP;
                        double2 vi = make_double2(0.0, 0.0), vj = vi;
                        if constexpr (BT == 1) {
                            if (in && oi[r] >= 0) vi = Up[(size_t)oi[r] * n + bp];
                            if (!diag && in && oj[r] >= 0) vj = Up[(size_t)oj[r] * n + bp];
                        } else {
                            vi = ui[r];
                            vj = uj[r];
                        }
                        const double2 ai = chi_cmul(ci[r], vi);
                        const double2 aj = diag ? ai : chi_cmul(cj[r], vj);
                        pl[0][sb][row] = t * ai.x;
                        pl[1][sb][row] = t * ai.y;
                        pl[2][sb][row] = aj.x;
                        pl[3][sb][row] = aj.y;
                    }
                    if constexpr (BT != 1) fetch(p0 + 16 < n ? p0 + 16 : 0);
                    __syncthreads();
                    // <4>: every wave multiplies its whole tile row in every k of the slice, so that no branch stands around the
                    // MFMAs (chi_orb_tiles); a dead row is zeros and is not written.  <1>: a team past its slice has nothing to add
                    if constexpr (BT == 1) {
                        if (valid && row_live) chi_orb_tiles<S, BT>(pl, ti, lane, accr, acci);
                    } else {
                        chi_orb_tiles<S, BT>(pl, ti, lane, accr, acci);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int tj = 0; tj < BT; ++tj) asm volatile("" : "+a"(accr[tj]), "+a"(acci[tj]));  // (see at the accumulators' declaration)
    if (!live || !row_live) return;
    // lane (q, c), register r: row q + 4 r, column c of the tile
    double2* out = part + ((size_t)ql * slices + sl) * mp * mp;
#pragma unroll
    for (int tj = 0; tj < BT; ++tj) {
        if (bj * RB + tj * 16 < m && !(diag && tj < ti)) {
            const int gj = bj * RB + tj * 16 + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gi = bi * RB + ti * 16 + (lane >> 4) + 4 * r;
                out[(size_t)gi * mp + gj] = make_double2(accr[tj][r], acci[tj][r]);
            }
        }
    }
}

// chi[q][perm[i]][perm[j]] = (the slices of part[q][.][i][j] in index order) / T / NK and its mirror, the conjugate: one thread per
// (q, i <= j) of the ascending list, perm its places in the caller's order.  The mirror's imaginary part is the difference from +0 and
// the diagonal's is +0.  grid: (elements / 256, vectors of the batch)
__global__ void __launch_bounds__(CHI_THREADS) chi_reduce_orb_kernel(const double2* __restrict__ part, int m, int mp, int64_t slices, double T,
                                                                     double nk, const int32_t* __restrict__ perm, double2* __restrict__ chi) {
    const int64_t e = (int64_t)blockIdx.x * CHI_THREADS + threadIdx.x;
    if (e >= (int64_t)m * m) return;
    const int i = (int)(e / m), j = (int)(e - (int64_t)i * m);
    if (i > j) return;
    const double2* p = part + (size_t)blockIdx.y * slices * mp * mp + (size_t)i * mp + j;
    double re = 0.0, im = 0.0;
    for (int64_t s = 0; s < slices; ++s) {
        const double2 v = p[(size_t)s * mp * mp];
        re += v.x;
        im += v.y;
    }
    re = re / T / nk;
    im = i == j ? 0.0 : im / T / nk;
    double2* out = chi + (size_t)blockIdx.y * m * m;
    const int ci = perm[i], cj = perm[j];
    out[(size_t)ci * m + cj] = make_double2(re, im);
    if (i != j) out[(size_t)cj * m + ci] = make_double2(re, 0.0 - im);
}

// ---- the orbital-resolved dynamic chi_0[i][j](q, omega + i eta) ----------------------------------------------
constexpr int CHI_OWC = 2;  // frequencies per register chunk of chi_orbital_dyn_kernel: 2 CHI_OWC BT accumulators and 2 CHI_OWC planes
                            // of X per item (DESIGN.md 31.2 has the compiler's report of 1, 2 and 4)

// chi_orb_tiles with one Y pair per tile and WC X pairs: the Y pairs of all BT tiles are read once per step of four b', then per
// frequency of the chunk its X pair and the four real products of zmfma_abh on its own accumulators.  pl: planes 0, 1 are Yr, Yi of the
// block's columns j, planes 2 + 2 w, 3 + 2 w are Xr, Xi of its rows i at frequency w of the chunk.  Nothing is guarded (chi_orb_tiles).
template <int S, int BT, int WC>
__device__ __forceinline__ void chi_orb_dyn_tiles(const double (*pl)[16][S], int ti, int lane, zd4 (&accr)[WC][BT], zd4 (&acci)[WC][BT]) {
#pragma unroll 1
    for (int q4 = 0; q4 < 4; ++q4) {  // (not unrolled: ZPanel's note on registers)
        const int kq = 4 * q4 + (lane >> 4);
        double yr[BT], yi[BT];
#pragma unroll
        for (int tj = 0; tj < BT; ++tj) {
            yr[tj] = pl[0][kq][tj * 16 + (lane & 15)];
            yi[tj] = pl[1][kq][tj * 16 + (lane & 15)];
        }
#pragma unroll
        for (int w = 0; w < WC; ++w) {
            const double xr = pl[2 + 2 * w][kq][ti * 16 + (lane & 15)], xi = pl[3 + 2 * w][kq][ti * 16 + (lane & 15)];
#pragma unroll
            for (int tj = 0; tj < BT; ++tj) zmfma_abh(xr, xi, yr[tj], yi[tj], accr[w][tj], acci[w][tj]);
        }
    }
}

// One complex-weighted rank-K update per (vector, frequency), K = (k, b, b') of a slice of k-points: sum X(omega) Y^H with Y = A,
// X = c A, c = g / (Delta + omega + i eta) = (g r x, -(g r eta)), x = Delta + omega, r = 1 / (x^2 + eta^2), g = chi_pair_difference and
// Delta = E[k][b] - E[k+q][b'] (one rounding).  The geometry, the staging and the walk of K are chi_orbital_kernel's; the sum is not
// Hermitian, so all nb^2 ordered blocks (bi, bj) = (blockIdx.y / nb, blockIdx.y % nb) and all tiles of a block are computed and
// written (tiles of the padding are multiplied and not written).  Frequencies go in register chunks of WC: per panel A is formed once
// (the Y planes), per frequency of the chunk X = c A goes to its own two planes and its own accumulators; a short last chunk is filled
// with copies of its last frequency, which are computed and not stored, so every frequency runs the same instructions.  g and Delta are
// made once per (k, b, b') and chunk where chi_orbital_kernel makes t, the WC complex weights from them go to LDS ahead of the panels
// that read them.  grid: (slices / KPW, nb^2, vectors of the batch x chunks of the pass); W: the nw frequencies of the pass, device
// memory.  One complex partial block per (q, omega, slice) goes to part[q][omega][slice][mp][mp].
template <int BT, int WC>
__global__ void __launch_bounds__(CHI_THREADS) chi_orbital_dyn_kernel(const double2* __restrict__ U, const double* __restrict__ E,
                                                                      const double* __restrict__ tab, ChiMesh g, int n,
                                                                      const int32_t* __restrict__ Q, const double2* __restrict__ D, double inv_t,
                                                                      const int32_t* __restrict__ orb, int m, int mp, int64_t ks, int64_t slices,
                                                                      const double* __restrict__ W, int nw, double eta,
                                                                      double2* __restrict__ part) {
    using Geo = ZPanel<BT>;  // (tbk_zmfma.h; an item is a slice)
    constexpr int RB = Geo::RB, KPW = Geo::KPW, TEAM = Geo::TEAM, S = Geo::S;
    static_assert(CHI_THREADS == Geo::THREADS, "the panel's workgroup");
    constexpr int STEP = TEAM / 16;                    // rows between the four a thread stages
    __shared__ double planes[KPW][2 + 2 * WC][16][S];  // Yr, Yi of the block's columns j; per frequency Xr, Xi of its rows i
    __shared__ double cw[KPW][WC][2][TEAM];            // c[omega][b'] of TEAM b' at once: one chi_pair_difference per (k, b, b')
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int team = BT == 1 ? wave : 0, tt = tid - team * TEAM;
    const int nb = mp / RB;
    const int bi = (int)blockIdx.y / nb, bj = (int)blockIdx.y - bi * nb;
    const int64_t sl = (int64_t)blockIdx.x * KPW + team;
    const int chunks = (nw + WC - 1) / WC;
    const int64_t ql = blockIdx.z / chunks;
    const int w0 = (int)(blockIdx.z - ql * chunks) * WC;
    const bool live = sl < slices;
    const int64_t k0 = live ? sl * ks : 0, k1 = live ? (k0 + ks < g.nk ? k0 + ks : g.nk) : 0;
    const double2* Dq = D ? D + (size_t)ql * n : nullptr;
    double(*pl)[16][S] = planes[team];
    double(*cwt)[2][TEAM] = cw[team];
    const int ti = BT == 1 ? 0 : wave;               // the wave's tile row
    const bool row_live = bi * RB + ti * 16 < m;     // (wave-uniform)
    const bool diag = bi == bj;
    const double eta2 = eta * eta;
    double om[WC];
#pragma unroll
    for (int w = 0; w < WC; ++w) om[w] = W[w0 + w < nw ? w0 + w : nw - 1];
    zd4 accr[WC][BT], acci[WC][BT];
#pragma unroll
    for (int w = 0; w < WC; ++w)
#pragma unroll
        for (int tj = 0; tj < BT; ++tj) accr[w][tj] = acci[w][tj] = zd4{0.0, 0.0, 0.0, 0.0};
    // (the accumulators' home is the AGPRs, as in chi_orbital_kernel: the empty statements behind the loops)
    const int sb = tt & 15, srow0 = tt >> 4;  // the b' (row of the panel) and the first orbital row this thread stages
    int oi[4], oj[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int pi = bi * RB + srow0 + r * STEP, pj = bj * RB + srow0 + r * STEP;
        oi[r] = pi < m ? orb[pi] : -1;
        oj[r] = pj < m ? orb[pj] : -1;
    }
    const int64_t items = g.nk * n;
    const int64_t kn = BT == 1 ? ks : k1 - k0;  // (<1>: a team past its slice keeps the barriers; <4>: one slice, its own length)
    for (int64_t kk = 0; kk < kn; ++kk) {
        const int64_t k = k0 + kk;
        const bool valid = BT != 1 || k < k1;  // (uniform in the team)
        const int64_t kp = valid ? chi_shifted(g, k, Q + ql * 3) : 0;
        const double2* Uk = U + (valid ? (size_t)k * n * n : 0);
        const double2* Up = U + (size_t)kp * n * n;
        const double *Ea = E + (valid ? (size_t)k * n : 0), *Eb = E + (size_t)kp * n;
        const double *fa = tab + (valid ? (size_t)k * n : 0), *ga = fa + items, *fb = tab + (size_t)kp * n, *gb = fb + items;
        // (<4> loads the thread's entries of U[k+q] one panel ahead, <1> where it stages: chi_orbital_kernel's note)
        double2 ui[4], uj[4];
        auto fetch = [&](int p0) {
            const int bp = p0 + sb;
            const bool in = valid && bp < n;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                ui[r] = uj[r] = make_double2(0.0, 0.0);
                if (in && oi[r] >= 0) ui[r] = Up[(size_t)oi[r] * n + bp];
                if (!diag && in && oj[r] >= 0) uj[r] = Up[(size_t)oj[r] * n + bp];
            }
        };
        if constexpr (BT != 1) fetch(0);
        for (int b = 0; b < n; ++b) {
            // conj(U[k][i][b]) D[i] of the thread's rows: one value per i and b
            double2 ci[4], cj[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                ci[r] = cj[r] = make_double2(0.0, 0.0);
                if (valid && oi[r] >= 0) {
                    const double2 u = Uk[(size_t)oi[r] * n + b];
                    ci[r] = make_double2(u.x, -u.y);
                    if (Dq) ci[r] = chi_cmul(ci[r], Dq[oi[r]]);
                }
                if (!diag && valid && oj[r] >= 0) {
                    const double2 u = Uk[(size_t)oj[r] * n + b];
                    cj[r] = make_double2(u.x, -u.y);
                    if (Dq) cj[r] = chi_cmul(cj[r], Dq[oj[r]]);
                }
            }
            const double ea = Ea[b], fav = fa[b], gav = ga[b];
            for (int s0 = 0; s0 < n; s0 += TEAM) {
                {
                    // (the panels that read the previous weights are behind their second barrier)
                    const int bp = s0 + tt;
                    const bool in = valid && bp < n;
                    const double gd = in ? chi_pair_difference(ea, fav, gav, Eb[bp], fb[bp], gb[bp], inv_t) : 0.0;
                    const double delta = in ? ea - Eb[bp] : 0.0;
#pragma unroll
                    for (int w = 0; w < WC; ++w) {
                        const double x = delta + om[w];
                        const double r = 1.0 / fma(x, x, eta2);
                        const double gr = gd * r;
                        cwt[w][0][tt] = gr * x;
                        cwt[w][1][tt] = -(gr * eta);
                    }
                }
                const int s1 = s0 + TEAM < n ? s0 + TEAM : n;
                for (int p0 = s0; p0 < s1; p0 += 16) {
                    __syncthreads();  // the previous panel has been read, the weights are written
                    const int bp = p0 + sb;
                    const bool in = valid && bp < n;
                    double2 c[WC];
#pragma unroll
                    for (int w = 0; w < WC; ++w) c[w] = make_double2(cwt[w][0][bp - s0], cwt[w][1][bp - s0]);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = srow0 + r * STEP;
                        double2 vi = make_double2(0.0, 0.0), vj = vi;
                        if constexpr (BT == 1) {
                            if (in && oi[r] >= 0) vi = Up[(size_t)oi[r] * n + bp];
                            if (!diag && in && oj[r] >= 0) vj = Up[(size_t)oj[r] * n + bp];
                        } else {
                            vi = ui[r];
                            vj = uj[r];
                        }
                        const double2 ai = chi_cmul(ci[r], vi);
                        const double2 aj = diag ? ai : chi_cmul(cj[r], vj);
                        pl[0][sb][row] = aj.x;
                        pl[1][sb][row] = aj.y;
#pragma unroll
                        for (int w = 0; w < WC; ++w) {
                            const double2 xw = chi_cmul(c[w], ai);
                            pl[2 + 2 * w][sb][row] = xw.x;
                            pl[3 + 2 * w][sb][row] = xw.y;
                        }
                    }
                    if constexpr (BT != 1) fetch(p0 + 16 < n ? p0 + 16 : 0);
                    __syncthreads();
                    // No branch around the MFMAs in either template (chi_orb_tiles' note; with two frequencies chi_orbital_kernel<1>'s
                    // guard costs 16 v_accvgpr moves per step here): a dead row and a team past its slice have staged zeros, which
                    // leave every sum as it is up to the sign of a zero, and the reduction adds the partials to +0
                    chi_orb_dyn_tiles<S, BT, WC>(pl, ti, lane, accr, acci);
                }
            }
        }
    }
#pragma unroll
    for (int w = 0; w < WC; ++w)
#pragma unroll
        for (int tj = 0; tj < BT; ++tj) asm volatile("" : "+a"(accr[w][tj]), "+a"(acci[w][tj]));  // (see at the accumulators' declaration)
    if (!live || !row_live) return;
    // lane (q, c), register r: row q + 4 r, column c of the tile
#pragma unroll
    for (int w = 0; w < WC; ++w) {
        if (w0 + w >= nw) continue;  // (a copy of the chunk's last frequency)
        double2* out = part + (((size_t)ql * nw + (w0 + w)) * slices + sl) * mp * mp;
#pragma unroll
        for (int tj = 0; tj < BT; ++tj) {
            if (bj * RB + tj * 16 < m) {
                const int gj = bj * RB + tj * 16 + (lane & 15);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int gi = bi * RB + ti * 16 + (lane >> 4) + 4 * r;
                    out[(size_t)gi * mp + gj] = make_double2(accr[w][tj][r], acci[w][tj][r]);
                }
            }
        }
    }
}

// chi[q][w_first + omega][perm[i]][perm[j]] = (0 - the slices of part[q][omega][.][i][j] in index order) / NK per component: one
// thread per (q, omega, i, j) of the ascending list over all m^2 entries, perm its places in the caller's order.  Four loads are in
// flight ahead of the ordered adds.  grid: (elements / 256, frequencies of the pass, vectors of the batch); chi: the batch's rows of
// [n_q][n_w][m][m]
__global__ void __launch_bounds__(CHI_THREADS) chi_reduce_orb_dyn_kernel(const double2* __restrict__ part, int m, int mp, int64_t slices,
                                                                         double nk, int64_t n_w, int64_t w_first,
                                                                         const int32_t* __restrict__ perm, double2* __restrict__ chi) {
    const int64_t e = (int64_t)blockIdx.x * CHI_THREADS + threadIdx.x;
    if (e >= (int64_t)m * m) return;
    const int i = (int)(e / m), j = (int)(e - (int64_t)i * m);
    const size_t block = (size_t)mp * mp;
    const double2* p = part + ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * slices * block + (size_t)i * mp + j;
    double re = 0.0, im = 0.0;
    int64_t s = 0;
    for (; s + 4 <= slices; s += 4) {
        const double2 v0 = p[(size_t)s * block], v1 = p[(size_t)(s + 1) * block], v2 = p[(size_t)(s + 2) * block], v3 = p[(size_t)(s + 3) * block];
        re += v0.x;
        im += v0.y;
        re += v1.x;
        im += v1.y;
        re += v2.x;
        im += v2.y;
        re += v3.x;
        im += v3.y;
    }
    for (; s < slices; ++s) {
        const double2 v = p[(size_t)s * block];
        re += v.x;
        im += v.y;
    }
    double2* out = chi + ((size_t)blockIdx.z * n_w + w_first + blockIdx.y) * m * m;
    out[(size_t)perm[i] * m + perm[j]] = make_double2((0.0 - re) / nk, (0.0 - im) / nk);
}

// ---- the four-index chi_0[i][l][j][m](q) ---------------------------------------------------------------------
constexpr int CHI_TEN_MAX = 16;  // selected orbitals, at most: X is 136 x 256 then
constexpr int CHI_TEN_RB = 64;   // rows and columns of a workgroup's block of X

// The MFMAs of stage B on one staged panel of 16 b: four steps of four b, the P pair of the wave's tile row read once per step, per
// tile the Q pair and the four real products of zmfma_ab (plain transpose, nothing conjugated).  As in chi_orb_tiles no tile is
// guarded: the loop holds ds_read_b64 and MFMA only, the padding is zeros.  pl: plane 0, the planes (Pr, Pi, Qr, Qi) are PLANE apart.
template <int S>
__device__ __forceinline__ void chi_ten_tiles(const double* pl, int ti, int lane, zd4 (&accr)[4], zd4 (&acci)[4]) {
    constexpr int PLANE = 16 * S;
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
        const double* at = pl + (4 * q4 + (lane >> 4)) * S + (lane & 15);
        const double pr = at[ti * 16], pi = at[PLANE + ti * 16];
#pragma unroll
        for (int tj = 0; tj < 4; ++tj) {
            const double qr = at[2 * PLANE + tj * 16], qi = at[3 * PLANE + tj * 16];
            zmfma_ab(pr, pi, qr, qi, accr[tj], acci[tj]);
        }
    }
}

// X[(i, j)][(l, m)] += sum over (k, b) of a slice of P[(i, j)][k b] Q[(l, m)][k b]: the factorised four-index bubble.  Rows of X: the
// pairs i <= j of the ascending selection in lexicographic order, m (m + 1) / 2 of them; columns: all pairs (l, m), l m + m.  A workgroup
// owns block (bi, bj) of 64 x 64, wave t its tile row t (ZPanel<4>'s geometry), over one slice of k-points.  Per k-point and panel of
// 16 bands b of U[k]:
//   stage A  wave t forms tile t of Q[(l, m)][b] = sum_b' W[(l, m)][b'] t[b'][b] for the block's 64 columns: b' in panels of 16 through
//            LDS (W = U'[l][b'] conj(U'[m][b']) made while staging with explicit fma, t one chi_pair_weight per thread), four steps of two
//            MFMAs (Re, Im: complex by real) per panel.  The Q of the other row blocks of the same columns is computed again there:
//            n / 128 of stage B's MFMAs per block (DESIGN.md 29.2 has the choice).
//   stage B  the tile goes to the Q planes [b][64], P = conj(U[k][i][b]) U[k][j][b] of the block's rows to the P planes, one barrier,
//            then chi_ten_tiles on the accumulators, which stay in registers over the slice.
// Every element walks k ascending, b ascending in panels of 16 from 0 (four per MFMA step), and inside Q the b' ascending likewise: a
// function of n alone.  Zeros stand beyond n, beyond the rows and beyond the columns.  One complex partial block goes to
// part[q][slice][tr][tc], padding included (tr, tc are multiples of 64: every store is inside).
// grid: (slices, blocks, vectors of the batch).  orb: the selected orbitals [m], ascending.
__global__ void __launch_bounds__(CHI_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) chi_tensor_kernel(const double2* __restrict__ U, const double* __restrict__ E,
                                                                 const double* __restrict__ tab, ChiMesh g, int n,
                                                                 const int32_t* __restrict__ Q, double inv_t, const int32_t* __restrict__ orb,
                                                                 int m, int64_t tr, int64_t tc, int64_t ks, int64_t slices,
                                                                 double2* __restrict__ part) {
    constexpr int S = ZPanel<4>::S, PLANE = 16 * S, TS = 18;
    static_assert(CHI_THREADS == ZPanel<4>::THREADS && CHI_TEN_RB == ZPanel<4>::RB, "the panel's workgroup");
    __shared__ double planes[4 * PLANE];  // Pr, Pi [b][rows of the block]; Qr, Qi [b][columns of the block]
    __shared__ double wpl[2 * PLANE];     // Wr, Wi [b'][columns of the block]
    __shared__ double tw[16 * TS];        // t[b'][b] of the two panels
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int cbk = (int)(tc / CHI_TEN_RB);
    const int bi = (int)blockIdx.y / cbk, bj = (int)blockIdx.y - bi * cbk;
    const int64_t sl = blockIdx.x, ql = blockIdx.z;
    const int64_t k0 = sl * ks, k1 = k0 + ks < g.nk ? k0 + ks : g.nk;
    const int mr = m * (m + 1) / 2, mc = m * m;
    const int sb = tid & 15, srow0 = tid >> 4;  // the band (row of a panel) and the first of the four rows / columns this thread stages
    int oi[4], oj[4], ol[4], om[4];             // the orbitals of its rows (i, j) and columns (l, m); -1: padding
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        int row = bi * CHI_TEN_RB + srow0 + 16 * r;
        oi[r] = oj[r] = ol[r] = om[r] = -1;
        if (row < mr) {
            int i = 0;
            while (row >= m - i) {
                row -= m - i;
                ++i;
            }
            oi[r] = orb[i];
            oj[r] = orb[i + row];
        }
        const int col = bj * CHI_TEN_RB + srow0 + 16 * r;
        if (col < mc) {
            ol[r] = orb[col / m];
            om[r] = orb[col % m];
        }
    }
    zd4 accr[4], acci[4];
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) accr[tj] = acci[tj] = zd4{0.0, 0.0, 0.0, 0.0};
    const int64_t items = g.nk * n;
    const int tbp = tid >> 4, tb = tid & 15;  // the (b', b) of the panel pair whose weight this thread makes
    // The accumulators' home.  chi_orbital_kernel's empty "+a" statements did not hold here: with the second set of MFMAs (stage A)
    // in the loop nest the compiler kept six of the eight accumulators in VGPRs and copied 48 words to and 48 from the AGPRs around
    // the 64 MFMAs of every panel, wherever the statements stood and with the loops nested or flat.  The kernel is
    // therefore bounded to two waves per SIMD (what its LDS allows anyway): 256 registers, no AGPRs, and the compiler selects the
    // MFMA that reads and writes its accumulator in VGPRs -- gfx950's register file is one, so the accumulators stay in place from
    // the first MFMA to the store and the built code has no v_accvgpr_* at all.  The k-points of the slice and the panels of b run
    // as ONE counter (k slow, b fast) and the four K steps are unrolled: one loop level carries the accumulators.
    const int panels = (n + 15) >> 4;
    const int64_t walks = (k1 - k0) * panels;
    int64_t k = k0;
    int b0 = 0;
    for (int64_t it = 0; it < walks; ++it) {
        const int64_t kp = chi_shifted(g, k, Q + ql * 3);
        const double2* Uk = U + (size_t)k * n * n;
        const double2* Up = U + (size_t)kp * n * n;
        const double *Ea = E + (size_t)k * n, *Eb = E + (size_t)kp * n;
        const double *fa = tab + (size_t)k * n, *ga = fa + items, *fb = tab + (size_t)kp * n, *gb = fb + items;
        // ---- stage A: the wave's tile of Q[(l, m)][b0 ... b0 + 16)
        zd4 qr = zd4{0.0, 0.0, 0.0, 0.0}, qi = qr;
        const int bw = b0 + tb;
        const bool bw_in = bw < n;
        const double ea = bw_in ? Ea[bw] : 0.0, fav = bw_in ? fa[bw] : 0.0, gav = bw_in ? ga[bw] : 0.0;
        for (int p0 = 0; p0 < n; p0 += 16) {
            __syncthreads();  // the previous panels have been read (W, t by stage A; P, Q by stage B of the panel before)
            const int bp = p0 + sb;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double wr = 0.0, wi = 0.0;
                if (bp < n && ol[r] >= 0) {
                    const double2 ul = Up[(size_t)ol[r] * n + bp], um = Up[(size_t)om[r] * n + bp];
                    wr = fma(ul.x, um.x, ul.y * um.y);     // U'[l] conj(U'[m])
                    wi = fma(ul.y, um.x, -(ul.x * um.y));
                }
                wpl[sb * S + srow0 + 16 * r] = wr;
                wpl[PLANE + sb * S + srow0 + 16 * r] = wi;
            }
            {
                const int bq = p0 + tbp;
                tw[tbp * TS + tb] = (bw_in && bq < n) ? chi_pair_weight(ea, fav, gav, Eb[bq], fb[bq], gb[bq], inv_t) : 0.0;
            }
            __syncthreads();
#pragma unroll 1
            for (int q4 = 0; q4 < 4; ++q4) {
                const int kq = 4 * q4 + (lane >> 4);
                const double wr = wpl[kq * S + wave * 16 + (lane & 15)], wi = wpl[PLANE + kq * S + wave * 16 + (lane & 15)];
                const double t = tw[kq * TS + (lane & 15)];
                qr = __builtin_amdgcn_mfma_f64_16x16x4f64(wr, t, qr, 0, 0, 0);
                qi = __builtin_amdgcn_mfma_f64_16x16x4f64(wi, t, qi, 0, 0, 0);
            }
        }
        // ---- stage B: lane (q, c), register r of the tile: column (l, m) = 16 wave + q + 4 r of the block, band c of the panel
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double* st = planes + 2 * PLANE + (lane & 15) * S + wave * 16 + (lane >> 4) + 4 * r;
            st[0] = qr[r];
            st[PLANE] = qi[r];
        }
        const int b = b0 + sb;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double pr = 0.0, pi = 0.0;
            if (b < n && oi[r] >= 0) {
                const double2 ui = Uk[(size_t)oi[r] * n + b], uj = Uk[(size_t)oj[r] * n + b];
                pr = fma(ui.x, uj.x, ui.y * uj.y);     // conj(U[i]) U[j]
                pi = fma(ui.x, uj.y, -(ui.y * uj.x));
            }
            planes[sb * S + srow0 + 16 * r] = pr;
            planes[PLANE + sb * S + srow0 + 16 * r] = pi;
        }
        __syncthreads();
        chi_ten_tiles<S>(planes, wave, lane, accr, acci);
        b0 += 16;
        if (b0 >= n) {
            b0 = 0;
            ++k;
        }
    }
    double2* out = part + ((size_t)ql * slices + sl) * (size_t)tr * (size_t)tc;
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) {
        const int gj = bj * CHI_TEN_RB + tj * 16 + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int gi = bi * CHI_TEN_RB + wave * 16 + (lane >> 4) + 4 * r;
            out[(size_t)gi * tc + gj] = make_double2(accr[tj][r], acci[tj][r]);
        }
    }
}

// chi[q][perm[i]][perm[l]][perm[j]][perm[m]] = (the slices of part[q][.][(i, j)][(l, m)] in index order) / T / NK and its mirror, the
// conjugate at [j][m][i][l]: one thread per (q, (i, l) <= (j, m)) of the ascending list, as rows and columns i m + l of the
// m^2 x m^2 matrix -- which has i <= j, the rows the kernel computes.  The mirror's imaginary part is the difference from +0 and the
// diagonal's is +0.  grid: (elements / 256, vectors of the batch)
__global__ void __launch_bounds__(CHI_THREADS) chi_reduce_ten_kernel(const double2* __restrict__ part, int m, int64_t tr, int64_t tc,
                                                                     int64_t slices, double T, double nk, const int32_t* __restrict__ perm,
                                                                     double2* __restrict__ chi) {
    const int64_t m2 = (int64_t)m * m;
    const int64_t e = (int64_t)blockIdx.x * CHI_THREADS + threadIdx.x;
    if (e >= m2 * m2) return;
    const int rr = (int)(e / m2), cc = (int)(e - (int64_t)rr * m2);
    if (rr > cc) return;
    const int i = rr / m, l = rr - i * m, j = cc / m, mm = cc - j * m;
    const int64_t row = (int64_t)i * m - (int64_t)i * (i - 1) / 2 + (j - i), col = (int64_t)l * m + mm;
    const size_t plane = (size_t)tr * (size_t)tc;
    const double2* p = part + (size_t)blockIdx.y * slices * plane + (size_t)row * tc + col;
    double re = 0.0, im = 0.0;
    for (int64_t s = 0; s < slices; ++s) {
        const double2 v = p[(size_t)s * plane];
        re += v.x;
        im += v.y;
    }
    re = re / T / nk;
    im = rr == cc ? 0.0 : im / T / nk;
    double2* out = chi + (size_t)blockIdx.y * m2 * m2;
    const int64_t ci = perm[i], cl = perm[l], cj = perm[j], cm = perm[mm];
    out[((ci * m + cl) * m + cj) * m + cm] = make_double2(re, im);
    if (rr != cc) out[((cj * m + cm) * m + ci) * m + cl] = make_double2(re, 0.0 - im);
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
// the frequencies of a dynamic call (n_w = 0: the static call)
struct ChiFreq {
    int64_t n_w = 0;
    const double* omega = nullptr;  // host
    double eta = 0.0;
};

// q[n_q][dim] reduced to [0, n_d) per axis, three entries per vector
int chi_reduce_q(int dim, const int32_t* mesh, int64_t n_q, const int64_t* q, std::vector<int32_t>* out) {
    try {
        out->assign((size_t)n_q * 3, 0);
    } catch (...) {
        tbk_set_error("cannot allocate the reduced vectors");
        return TBK_ERR_MEMORY;
    }
    for (int64_t r = 0; r < n_q; ++r)
        for (int d = 0; d < dim; ++d) {
            const int64_t nd = mesh[d];
            (*out)[(size_t)r * 3 + d] = (int32_t)(((q[r * dim + d] % nd) + nd) % nd);
        }
    return TBK_OK;
}

int chi_launch_fermi(hipStream_t s, const ChiPlan& L, SpanRecorder* ev, const double* d_E, double mu, double T, double* d_tab) {
    const int64_t items = L.mesh.nk * L.n;
    if (ev) ev->start(0);
    hipLaunchKernelGGL(chi_fermi_kernel, dim3((unsigned)((items + CHI_THREADS - 1) / CHI_THREADS)), dim3(CHI_THREADS), 0, s, d_E, items, mu, T,
                       d_tab);
    if (ev) ev->stop();
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

// nq vectors (at most L.batch): d_Q their reduced entries, d_D their phases (or NULL), d_chi their results
int chi_launch_batch(hipStream_t s, const ChiPlan& L, SpanRecorder* ev, const double* d_U, const double* d_E, const double* d_tab,
                     const int32_t* d_Q, const double* d_D, int64_t nq, double T, double* d_part, double* d_chi) {
    const double inv_t = 1.0 / T;
    const int64_t nk = L.mesh.nk;
    if (ev) ev->start(1);
    if (L.bt == 0) {
        hipLaunchKernelGGL(chi_pair_kernel, dim3((unsigned)((nk + 3) / 4), 1, (unsigned)nq), dim3(CHI_THREADS), 0, s, d_E, d_tab, L.mesh, L.n, d_Q,
                           inv_t, d_part);
    } else if (L.bt == 1) {
        hipLaunchKernelGGL((chi_overlap_kernel<1, false>), dim3((unsigned)((nk + 3) / 4), 1, (unsigned)nq), dim3(CHI_THREADS), 0, s,
                           reinterpret_cast<const double2*>(d_U), d_E, d_tab, L.mesh, L.n, d_Q, reinterpret_cast<const double2*>(d_D), inv_t,
                           L.blocks, d_part, ChiDyn());
    } else {
        hipLaunchKernelGGL((chi_overlap_kernel<4, false>), dim3((unsigned)nk, (unsigned)L.blocks, (unsigned)nq), dim3(CHI_THREADS), 0, s,
                           reinterpret_cast<const double2*>(d_U), d_E, d_tab, L.mesh, L.n, d_Q, reinterpret_cast<const double2*>(d_D), inv_t,
                           L.blocks, d_part, ChiDyn());
    }
    if (ev) ev->stop();
    TBK_HIP(hipGetLastError());
    if (ev) ev->start(2);
    hipLaunchKernelGGL(chi_reduce_kernel, dim3((unsigned)nq), dim3(CHI_THREADS), 0, s, d_part, nk * L.blocks, T, (double)nk, d_chi);
    if (ev) ev->stop();
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

// the dynamic call's: nq vectors (at most L.batch), every pass of the frequencies d_W[L.n_w]; d_chi: their rows of [.][L.n_w] complex.
// The spans are the static call's: 1 = the overlaps with the dynamic epilogue (or the pair kernel), 2 = the reduction.
int chi_launch_dyn_batch(hipStream_t s, const ChiPlan& L, SpanRecorder* ev, const double* d_U, const double* d_E, const double* d_tab,
                         const int32_t* d_Q, const double* d_D, int64_t nq, double T, const double* d_W, double eta, double* d_part,
                         double* d_chi) {
    const double inv_t = 1.0 / T;
    const int64_t nk = L.mesh.nk;
    for (int64_t w0 = 0; w0 < L.n_w; w0 += L.w_pass) {
        ChiDyn dyn;
        dyn.W = d_W + w0;
        dyn.nw = (int)std::min(L.w_pass, L.n_w - w0);
        dyn.eta = eta;
        dyn.part = reinterpret_cast<double2*>(d_part);
        if (ev) ev->start(1);
        if (L.bt == 0) {
            hipLaunchKernelGGL(chi_pair_dyn_kernel, dim3((unsigned)((nk + 3) / 4), 1, (unsigned)nq), dim3(CHI_THREADS), 0, s, d_E, d_tab, L.mesh, L.n,
                               d_Q, inv_t, dyn);
        } else if (L.bt == 1) {
            hipLaunchKernelGGL((chi_overlap_kernel<1, true>), dim3((unsigned)((nk + 3) / 4), 1, (unsigned)nq), dim3(CHI_THREADS), 0, s,
                               reinterpret_cast<const double2*>(d_U), d_E, d_tab, L.mesh, L.n, d_Q, reinterpret_cast<const double2*>(d_D), inv_t,
                               L.blocks, nullptr, dyn);
        } else {
            hipLaunchKernelGGL((chi_overlap_kernel<4, true>), dim3((unsigned)nk, (unsigned)L.blocks, (unsigned)nq), dim3(CHI_THREADS), 0, s,
                               reinterpret_cast<const double2*>(d_U), d_E, d_tab, L.mesh, L.n, d_Q, reinterpret_cast<const double2*>(d_D), inv_t,
                               L.blocks, nullptr, dyn);
        }
        if (ev) ev->stop();
        TBK_HIP(hipGetLastError());
        if (ev) ev->start(2);
        hipLaunchKernelGGL(chi_reduce_dyn_kernel, dim3((unsigned)dyn.nw, (unsigned)nq), dim3(CHI_THREADS), 0, s, dyn.part, nk * L.blocks, (double)nk,
                           L.n_w, w0, reinterpret_cast<double2*>(d_chi));
        if (ev) ev->stop();
        TBK_HIP(hipGetLastError());
    }
    return TBK_OK;
}

// ---- the orbital-resolved call's plan, arguments and launches ----------------------------------------------------------------------
constexpr int64_t CHI_ORB_AMORTISE = 1024;  // (b, b') pairs a slice walks at least per register-resident block
constexpr int64_t CHI_ORB_SLICES = 1024;    // slices of one vector, about: four workgroups (or one of four slices) per compute unit

// the library's slice length, a function of (NK, n_orb) alone -- not of the selection, the vectors, the batch or the handles, so that
// the bits of an element are those of any call that contains it: long enough to walk CHI_ORB_AMORTISE pairs per block held in
// registers, short enough for about CHI_ORB_SLICES slices per vector, and long enough that four vectors' partials of the full matrix
// fit the budget
int64_t chi_orb_slice(int64_t nk, int n_orb) {
    const int64_t n2 = (int64_t)n_orb * n_orb, np = ((int64_t)n_orb + 63) / 64 * 64;
    const int64_t amortise = (CHI_ORB_AMORTISE + n2 - 1) / n2, fill = (nk + CHI_ORB_SLICES - 1) / CHI_ORB_SLICES;
    const int64_t most = std::max<int64_t>(1, (int64_t)(CHI_PART_BUDGET / 4 / (sizeof(double2) * (size_t)np * (size_t)np)));
    return std::min(nk, std::max(std::max(amortise, fill), (nk + most - 1) / most));
}

// the one place that chooses: template, blocks, slice length (k_slice = 0: the library's), slices, batch from the bytes the partials
// may take (0: the budget)
void chi_orb_plan_sizes(int64_t nk, int n_orb, int m, int64_t n_q, size_t mem, int64_t k_slice, ChiPlan* L) {
    L->n = n_orb;
    L->m = m;
    L->bt = m <= 16 ? 1 : 4;
    const int rb = 16 * L->bt;
    const int64_t nb = (m + rb - 1) / rb;
    L->mp = (int)(nb * rb);
    L->blocks = nb * (nb + 1) / 2;
    L->ks = k_slice > 0 ? std::min(k_slice, nk) : chi_orb_slice(nk, n_orb);
    L->slices = (nk + L->ks - 1) / L->ks;
    const size_t per_q = (size_t)L->slices * L->mp * L->mp * sizeof(double2);
    const size_t room = mem == 0 ? CHI_PART_BUDGET : mem;
    L->batch = std::max<int64_t>(0, std::min<int64_t>(std::min(n_q, CHI_MAX_BATCH), (int64_t)(room / per_q)));
    L->batches = L->batch == 0 ? 0 : (n_q + L->batch - 1) / L->batch;
}

// the orbital-resolved dynamic call's: template, all nb^2 blocks, chi_orb_slice's slice length (a function of (NK, n_orb) alone; k_slice =
// 0: the library's), and chi_dyn_plan_sizes' split with 16 slices mp^2 bytes per (q, omega): all frequencies of a vector in one launch
// when they fit (then as many vectors as fit, and as the grid's z takes with their register chunks), else one vector per batch and the
// frequencies in passes, whole chunks of CHI_OWC when one fits
void chi_orb_dyn_plan_sizes(int64_t nk, int n_orb, int m, int64_t n_q, int64_t n_w, size_t mem, int64_t k_slice, ChiPlan* L) {
    L->n = n_orb;
    L->m = m;
    L->bt = m <= 16 ? 1 : 4;
    const int rb = 16 * L->bt;
    const int64_t nb = (m + rb - 1) / rb;
    L->mp = (int)(nb * rb);
    L->blocks = nb * nb;
    L->ks = k_slice > 0 ? std::min(k_slice, nk) : chi_orb_slice(nk, n_orb);
    L->slices = (nk + L->ks - 1) / L->ks;
    L->n_w = n_w;
    const size_t per_qw = (size_t)L->slices * L->mp * L->mp * sizeof(double2);
    const size_t room = mem == 0 ? CHI_PART_BUDGET : mem;
    const int64_t fit = (int64_t)std::min<size_t>(room / per_qw, (size_t)1 << 62);  // (q, omega) pairs whose partials fit
    if (fit >= n_w) {
        const int64_t chunks = (n_w + CHI_OWC - 1) / CHI_OWC;
        L->w_pass = n_w;
        L->batch = std::min(std::min<int64_t>(std::min(n_q, CHI_MAX_BATCH), fit / n_w), CHI_GRID_YZ / chunks);
    } else {
        L->w_pass = fit >= CHI_OWC ? fit / CHI_OWC * CHI_OWC : fit;
        L->batch = fit >= 1 ? 1 : 0;
    }
    L->passes = L->w_pass == 0 ? 0 : (n_w + L->w_pass - 1) / L->w_pass;
    L->batches = L->batch == 0 ? 0 : (n_q + L->batch - 1) / L->batch;
}

constexpr int64_t CHI_TEN_AMORTISE = 8;   // panels of 16 b a slice walks at least per register-resident block (64 KiB of partials)
constexpr int64_t CHI_TEN_SLICES = 256;   // slices of one vector, about: with up to 12 blocks each, workgroups for every compute unit

// the four-index call's slice length, a function of (NK, n_orb) alone as chi_orb_slice is and for its reason: long enough to walk
// CHI_TEN_AMORTISE panels per block, short enough for about CHI_TEN_SLICES slices, and long enough that two vectors' partials of the
// largest selection (16 orbitals: 192 x 256 padded) fit the budget
int64_t chi_ten_slice(int64_t nk, int n_orb) {
    const int64_t panels = ((int64_t)n_orb + 15) / 16;
    const int64_t amortise = (CHI_TEN_AMORTISE + panels - 1) / panels, fill = (nk + CHI_TEN_SLICES - 1) / CHI_TEN_SLICES;
    const int64_t most = (int64_t)(CHI_PART_BUDGET / 2 / (sizeof(double2) * 192 * 256));
    return std::min(nk, std::max(std::max(amortise, fill), (nk + most - 1) / most));
}

// the one place that chooses for the four-index call: blocks, slice length (k_slice = 0: the library's), slices, batch
void chi_ten_plan_sizes(int64_t nk, int n_orb, int m, int64_t n_q, size_t mem, int64_t k_slice, ChiPlan* L) {
    L->n = n_orb;
    L->m = m;
    L->bt = 4;
    L->tr = ((int64_t)m * (m + 1) / 2 + CHI_TEN_RB - 1) / CHI_TEN_RB * CHI_TEN_RB;
    L->tc = ((int64_t)m * m + CHI_TEN_RB - 1) / CHI_TEN_RB * CHI_TEN_RB;
    L->blocks = (L->tr / CHI_TEN_RB) * (L->tc / CHI_TEN_RB);
    L->ks = k_slice > 0 ? std::min(k_slice, nk) : chi_ten_slice(nk, n_orb);
    L->slices = (nk + L->ks - 1) / L->ks;
    const size_t room = mem == 0 ? CHI_PART_BUDGET : mem;
    L->batch = std::max<int64_t>(0, std::min<int64_t>(std::min(n_q, CHI_MAX_BATCH), (int64_t)(room / L->per_q())));
    L->batches = L->batch == 0 ? 0 : (n_q + L->batch - 1) / L->batch;
}

// The plan of n_q vectors on a mesh of nk points: n_w frequencies (0: static), m selected orbitals (0: the scalar calls; k_slice
// is theirs) of the orbital-resolved or, with `tensor`, the four-index call; mem: the bytes the partials may take (0: the budget)
int chi_plan(int dim, const int32_t* mesh, int64_t nk, int n_orb, int64_t n_q, int64_t n_w, int m, bool tensor, bool matrix_elements,
             size_t mem, int64_t k_slice, ChiPlan* out) {
    ChiPlan L;
    L.mesh.n[0] = mesh[0];
    L.mesh.n[1] = mesh[1];
    L.mesh.n[2] = dim == 3 ? mesh[2] : 1;
    L.mesh.nk = nk;
    L.n = n_orb;
    TBK_ARG(nk <= CHI_MAX_NK, "the susceptibility takes meshes of up to 2^23 points");
    L.n_w = n_w;
    if (m > 0 && tensor)
        chi_ten_plan_sizes(nk, n_orb, m, n_q, mem, k_slice, &L);
    else if (m > 0 && n_w > 0)
        chi_orb_dyn_plan_sizes(nk, n_orb, m, n_q, n_w, mem, k_slice, &L);
    else if (m > 0)
        chi_orb_plan_sizes(nk, n_orb, m, n_q, mem, k_slice, &L);
    else if (n_w == 0)
        chi_plan_sizes(nk, n_orb, n_q, matrix_elements, mem, &L.bt, &L.blocks, &L.batch, &L.batches);
    else
        chi_dyn_plan_sizes(nk, n_orb, n_q, n_w, matrix_elements, mem, &L.bt, &L.blocks, &L.batch, &L.batches, &L.w_pass, &L.passes);
    if (L.batch < 1) {
        if (m > 0)
            tbk_set_error("the partial sums of one %s susceptibility vector%s need %zu bytes of device memory",
                          tensor ? "four-index" : "orbital-resolved", n_w == 0 ? "" : " at one frequency", L.per_q());
        else
            tbk_set_error("the partial sums of one susceptibility vector%s need %zu bytes of device memory", n_w == 0 ? "" : " at one frequency",
                          L.per_q());
        return TBK_ERR_MEMORY;
    }
    *out = L;
    return TBK_OK;
}

// the selection of an orbital-resolved or four-index call (off: the scalar calls)
struct ChiOrb {
    bool on = false;
    int m = 0;
    const int32_t* orbitals = nullptr;  // host [m] or NULL: all of them in order (m = n_orb)
    bool tensor = false;                // the four-index call: m <= CHI_TEN_MAX, [m][m][m][m] per vector
};

// lists[0 .. m): the selection in ascending order; lists[m .. 2 m): the place of each in the caller's order
// (a scalar call: none)
int chi_orb_lists(const ChiOrb& ob, int n_orb, std::vector<int32_t>* lists) {
    if (!ob.on) return TBK_OK;
    TBK_ARG(ob.m >= 1 && ob.m <= n_orb, "m < 1 or more selected orbitals than the model has");
    TBK_ARG(!ob.tensor || ob.m <= CHI_TEN_MAX, "the four-index susceptibility takes up to 16 selected orbitals");
    TBK_ARG(ob.orbitals != nullptr || ob.m == n_orb, "orbitals is NULL and m is not n_orb");
    try {
        lists->assign((size_t)ob.m * 2, 0);
    } catch (...) {
        tbk_set_error("cannot allocate the orbital list");
        return TBK_ERR_MEMORY;
    }
    for (int p = 0; p < ob.m; ++p) {
        const int32_t o = ob.orbitals ? ob.orbitals[p] : p;
        TBK_ARG(o >= 0 && o < n_orb, "an orbital index is out of range");
        (*lists)[(size_t)ob.m + p] = p;
    }
    int32_t* perm = lists->data() + ob.m;
    const int32_t* given = ob.orbitals;
    std::sort(perm, perm + ob.m, [given](int32_t a, int32_t b) { return given ? given[a] < given[b] : a < b; });
    for (int p = 0; p < ob.m; ++p) (*lists)[(size_t)p] = given ? given[perm[p]] : p;
    for (int p = 1; p < ob.m; ++p) TBK_ARG((*lists)[(size_t)p] != (*lists)[(size_t)p - 1], "an orbital index is repeated");
    return TBK_OK;
}

// the orbital-resolved call's: nq vectors (at most L.batch); d_lists: chi_orb_lists' on the device; d_chi: their [.][m][m] complex
int chi_launch_orb_batch(hipStream_t s, const ChiPlan& L, SpanRecorder* ev, const double* d_U, const double* d_E, const double* d_tab,
                         const int32_t* d_Q, const double* d_D, const int32_t* d_lists, int64_t nq, double T, double* d_part, double* d_chi) {
    const double inv_t = 1.0 / T;
    const int64_t elements = (int64_t)L.m * L.m;
    const double2* D = reinterpret_cast<const double2*>(d_D);
    if (ev) ev->start(1);
    if (L.bt == 1) {
        hipLaunchKernelGGL((chi_orbital_kernel<1>), dim3((unsigned)((L.slices + 3) / 4), 1, (unsigned)nq), dim3(CHI_THREADS), 0, s,
                           reinterpret_cast<const double2*>(d_U), d_E, d_tab, L.mesh, L.n, d_Q, D, inv_t, d_lists, L.m, L.mp, L.ks, L.slices,
                           reinterpret_cast<double2*>(d_part));
    } else {
        hipLaunchKernelGGL((chi_orbital_kernel<4>), dim3((unsigned)L.slices, (unsigned)L.blocks, (unsigned)nq), dim3(CHI_THREADS), 0, s,
                           reinterpret_cast<const double2*>(d_U), d_E, d_tab, L.mesh, L.n, d_Q, D, inv_t, d_lists, L.m, L.mp, L.ks, L.slices,
                           reinterpret_cast<double2*>(d_part));
    }
    if (ev) ev->stop();
    TBK_HIP(hipGetLastError());
    if (ev) ev->start(2);
    hipLaunchKernelGGL(chi_reduce_orb_kernel, dim3((unsigned)((elements + CHI_THREADS - 1) / CHI_THREADS), (unsigned)nq), dim3(CHI_THREADS), 0, s,
                       reinterpret_cast<const double2*>(d_part), L.m, L.mp, L.slices, T, (double)L.mesh.nk, d_lists + L.m,
                       reinterpret_cast<double2*>(d_chi));
    if (ev) ev->stop();
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

// the orbital-resolved dynamic call's: nq vectors (at most L.batch), every pass of the frequencies d_W[L.n_w]; d_chi: their
// [.][L.n_w][m][m] complex.  The spans are the static call's: 1 = the rank-K update, 2 = the reduction.
int chi_launch_orb_dyn_batch(hipStream_t s, const ChiPlan& L, SpanRecorder* ev, const double* d_U, const double* d_E, const double* d_tab,
                             const int32_t* d_Q, const double* d_D, const int32_t* d_lists, int64_t nq, double T, const double* d_W, double eta,
                             double* d_part, double* d_chi) {
    const double inv_t = 1.0 / T;
    const int64_t elements = (int64_t)L.m * L.m;
    const double2* D = reinterpret_cast<const double2*>(d_D);
    for (int64_t w0 = 0; w0 < L.n_w; w0 += L.w_pass) {
        const int nw = (int)std::min(L.w_pass, L.n_w - w0);
        const int64_t chunks = (nw + CHI_OWC - 1) / CHI_OWC;
        if (ev) ev->start(1);
        if (L.bt == 1) {
            hipLaunchKernelGGL((chi_orbital_dyn_kernel<1, CHI_OWC>), dim3((unsigned)((L.slices + 3) / 4), 1, (unsigned)(nq * chunks)),
                               dim3(CHI_THREADS), 0, s, reinterpret_cast<const double2*>(d_U), d_E, d_tab, L.mesh, L.n, d_Q, D, inv_t, d_lists, L.m,
                               L.mp, L.ks, L.slices, d_W + w0, nw, eta, reinterpret_cast<double2*>(d_part));
        } else {
            hipLaunchKernelGGL((chi_orbital_dyn_kernel<4, CHI_OWC>), dim3((unsigned)L.slices, (unsigned)L.blocks, (unsigned)(nq * chunks)),
                               dim3(CHI_THREADS), 0, s, reinterpret_cast<const double2*>(d_U), d_E, d_tab, L.mesh, L.n, d_Q, D, inv_t, d_lists, L.m,
                               L.mp, L.ks, L.slices, d_W + w0, nw, eta, reinterpret_cast<double2*>(d_part));
        }
        if (ev) ev->stop();
        TBK_HIP(hipGetLastError());
        if (ev) ev->start(2);
        hipLaunchKernelGGL(chi_reduce_orb_dyn_kernel, dim3((unsigned)((elements + CHI_THREADS - 1) / CHI_THREADS), (unsigned)nw, (unsigned)nq),
                           dim3(CHI_THREADS), 0, s, reinterpret_cast<const double2*>(d_part), L.m, L.mp, L.slices, (double)L.mesh.nk, L.n_w, w0,
                           d_lists + L.m, reinterpret_cast<double2*>(d_chi));
        if (ev) ev->stop();
        TBK_HIP(hipGetLastError());
    }
    return TBK_OK;
}

// the four-index call's: nq vectors (at most L.batch); d_lists: chi_orb_lists' on the device; d_chi: their [.][m][m][m][m] complex
int chi_launch_ten_batch(hipStream_t s, const ChiPlan& L, SpanRecorder* ev, const double* d_U, const double* d_E, const double* d_tab,
                         const int32_t* d_Q, const int32_t* d_lists, int64_t nq, double T, double* d_part, double* d_chi) {
    const int64_t elements = (int64_t)L.m * L.m * L.m * L.m;
    if (ev) ev->start(1);
    hipLaunchKernelGGL(chi_tensor_kernel, dim3((unsigned)L.slices, (unsigned)L.blocks, (unsigned)nq), dim3(CHI_THREADS), 0, s,
                       reinterpret_cast<const double2*>(d_U), d_E, d_tab, L.mesh, L.n, d_Q, 1.0 / T, d_lists, L.m, L.tr, L.tc, L.ks, L.slices,
                       reinterpret_cast<double2*>(d_part));
    if (ev) ev->stop();
    TBK_HIP(hipGetLastError());
    if (ev) ev->start(2);
    hipLaunchKernelGGL(chi_reduce_ten_kernel, dim3((unsigned)((elements + CHI_THREADS - 1) / CHI_THREADS), (unsigned)nq), dim3(CHI_THREADS), 0, s,
                       reinterpret_cast<const double2*>(d_part), L.m, L.tr, L.tc, L.slices, T, (double)L.mesh.nk, d_lists + L.m,
                       reinterpret_cast<double2*>(d_chi));
    if (ev) ev->stop();
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

// The Fermi tables once, then all batches of n_q vectors whose reduced entries (and phases) are on the device, by the plan's kind:
// d_chi [n_q], [n_q][L.n_w] complex with the frequencies d_W of a dynamic call, or [n_q][m][m] complex with the orbital-resolved
// call's d_lists (with both [n_q][L.n_w][m][m] complex), or [n_q][m][m][m][m] complex with the four-index call's
int chi_launch_all(hipStream_t s, const ChiPlan& L, SpanRecorder* ev, const double* d_U, const double* d_E, double* d_tab, const int32_t* d_Q,
                   const double* d_D, const int32_t* d_lists, int64_t n_q, double mu, double T, const double* d_W, double eta, double* d_part,
                   double* d_chi) {
    TBK_CHECK(chi_launch_fermi(s, L, ev, d_E, mu, T, d_tab));
    for (int64_t q0 = 0; q0 < n_q; q0 += L.batch) {
        const int64_t nq = std::min(L.batch, n_q - q0);
        const int32_t* Q = d_Q + q0 * 3;
        const double* D = d_D ? d_D + (size_t)q0 * L.n * 2 : nullptr;
        if (L.tr > 0)
            TBK_CHECK(chi_launch_ten_batch(s, L, ev, d_U, d_E, d_tab, Q, d_lists, nq, T, d_part,
                                           d_chi + (size_t)q0 * L.m * L.m * L.m * L.m * 2));
        else if (L.m > 0 && L.n_w > 0)
            TBK_CHECK(chi_launch_orb_dyn_batch(s, L, ev, d_U, d_E, d_tab, Q, D, d_lists, nq, T, d_W, eta, d_part,
                                               d_chi + (size_t)q0 * L.n_w * L.m * L.m * 2));
        else if (L.m > 0)
            TBK_CHECK(chi_launch_orb_batch(s, L, ev, d_U, d_E, d_tab, Q, D, d_lists, nq, T, d_part, d_chi + (size_t)q0 * L.m * L.m * 2));
        else if (L.n_w > 0)
            TBK_CHECK(chi_launch_dyn_batch(s, L, ev, d_U, d_E, d_tab, Q, D, nq, T, d_W, eta, d_part, d_chi + (size_t)q0 * L.n_w * 2));
        else
            TBK_CHECK(chi_launch_batch(s, L, ev, d_U, d_E, d_tab, Q, D, nq, T, d_part, d_chi + q0));
    }
    return TBK_OK;
}

int chi_check(double T, int64_t n_q, const int64_t* q, const double* chi_out, int n_orb) {
    TBK_ARG(std::isfinite(T) && T > 0.0, "the temperature is not finite or not positive");
    TBK_ARG(n_q >= 1, "n_q < 1");
    TBK_ARG(q != nullptr && chi_out != nullptr, "q / chi is NULL");
    TBK_ARG(n_orb >= 1 && n_orb <= CHI_MAX_ORB, "n_orb < 1 or more than 16320 orbitals");
    return TBK_OK;
}

int chi_check_frequencies(int64_t n_w, const double* omega, double eta, bool orbital) {
    if (orbital)
        return pair_check_frequencies(n_w, CHI_ORB_MAX_NW, omega, eta,
                                      "the orbital-resolved dynamic susceptibility takes up to 65535 frequencies per call");
    return pair_check_frequencies(n_w, CHI_MAX_NW, omega, eta, "the dynamic susceptibility takes up to 2^23 frequencies per call");
}

constexpr const char* CHI_FAMILY = "the susceptibility";

// the bytes of one vector's result: a double, n_w complex numbers, the m x m complex matrix (one per frequency of an orbital-resolved
// dynamic call) or the m x m x m x m complex tensor
size_t chi_out_per_q(const ChiFreq& fr, const ChiOrb& ob) {
    if (ob.on && ob.tensor) return (size_t)ob.m * ob.m * ob.m * ob.m * sizeof(double2);
    if (ob.on && fr.n_w != 0) return (size_t)fr.n_w * ob.m * ob.m * sizeof(double2);
    return ob.on ? (size_t)ob.m * ob.m * sizeof(double2) : fr.n_w == 0 ? sizeof(double) : (size_t)fr.n_w * sizeof(double2);
}

}  // namespace

extern "C" int tbk_chi_plan(int64_t nk, int n_orb, int64_t n_q, int matrix_elements, int64_t part_bytes, int64_t* out) {
    TBK_ARG(nk >= 1 && n_orb >= 1 && n_orb <= CHI_MAX_ORB && n_q >= 1 && part_bytes >= 0 && out != nullptr,
            "nk / n_orb / n_q < 1, more than 16320 orbitals, part_bytes < 0 or out is NULL");
    int bt = 0;
    chi_plan_sizes(nk, n_orb, n_q, matrix_elements != 0, (size_t)part_bytes, &bt, &out[1], &out[2], &out[3]);
    out[0] = bt;
    return TBK_OK;
}

// the kernels on a caller's eigensystem: chi_out double [n_q], with frequencies complex [n_q][n_w], with a selection complex
// [n_q][m][m]; mem: the bytes the partials may take (0: the budget), k_slice: the orbital-resolved call's slice (0: the library's)
static int chi_from_eigensystem(int device, int dim, const int32_t* mesh, int n_orb, const double* E, const double* U, double mu, double T,
                         int64_t n_q, const int64_t* q, const double* phases, const ChiFreq& fr, const ChiOrb& ob, size_t mem, int64_t k_slice,
                         double* chi_out) {
    int64_t nk = 0;
    TBK_CHECK(tetra_check_mesh(dim, mesh, OCC_MESH, &nk));
    TBK_ARG(E != nullptr, "E is NULL");
    TBK_ARG(std::isfinite(mu), "the chemical potential is not finite");
    TBK_CHECK(chi_check(T, n_q, q, chi_out, n_orb));
    if (fr.n_w != 0) TBK_CHECK(chi_check_frequencies(fr.n_w, fr.omega, fr.eta, ob.on));
    TBK_ARG(U != nullptr || !ob.on, "U is NULL: the orbital-resolved susceptibility needs the eigenvectors");
    TBK_ARG(U != nullptr || phases == nullptr, "phases without eigenvectors");
    std::vector<int32_t> h_lists;
    TBK_CHECK(chi_orb_lists(ob, n_orb, &h_lists));
    TBK_CHECK(tetra_check_device(device));
    ChiPlan L;
    TBK_CHECK(chi_plan(dim, mesh, nk, n_orb, n_q, fr.n_w, ob.m, ob.tensor, U != nullptr, mem, k_slice, &L));
    const size_t out_bytes = (size_t)n_q * chi_out_per_q(fr, ob);
    std::vector<int32_t> h_Q;
    TBK_CHECK(chi_reduce_q(dim, mesh, n_q, q, &h_Q));
    const size_t e_bytes = (size_t)nk * n_orb * sizeof(double), u_bytes = (size_t)nk * n_orb * n_orb * sizeof(double2);
    const size_t d_bytes = (size_t)n_q * n_orb * sizeof(double2), l_bytes = h_lists.size() * sizeof(int32_t);
    DevBuf d_E, d_U, d_tab, d_Q, d_lists, d_D, d_W, d_part, d_chi;
    TBK_CHECK(d_E.reserve(e_bytes));
    TBK_CHECK(d_tab.reserve(2 * e_bytes));
    if (U) TBK_CHECK(mesh_reserve(d_U, u_bytes, CHI_FAMILY, "the eigenvectors of the whole mesh"));
    TBK_CHECK(d_Q.reserve(h_Q.size() * sizeof(int32_t)));
    if (l_bytes) TBK_CHECK(d_lists.reserve(l_bytes));
    if (phases) TBK_CHECK(d_D.reserve(d_bytes));
    TBK_CHECK(d_part.reserve(L.part_bytes()));
    TBK_CHECK(d_chi.reserve(out_bytes));
    if (fr.n_w != 0) {
        TBK_CHECK(d_W.reserve((size_t)fr.n_w * sizeof(double)));
        TBK_HIP(hipMemcpy(d_W.ptr, fr.omega, (size_t)fr.n_w * sizeof(double), hipMemcpyHostToDevice));
    }
    TBK_HIP(hipMemcpy(d_E.ptr, E, e_bytes, hipMemcpyHostToDevice));
    if (U) TBK_HIP(hipMemcpy(d_U.ptr, U, u_bytes, hipMemcpyHostToDevice));
    TBK_HIP(hipMemcpy(d_Q.ptr, h_Q.data(), h_Q.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    if (l_bytes) TBK_HIP(hipMemcpy(d_lists.ptr, h_lists.data(), l_bytes, hipMemcpyHostToDevice));
    if (phases) TBK_HIP(hipMemcpy(d_D.ptr, phases, d_bytes, hipMemcpyHostToDevice));
    TBK_CHECK(chi_launch_all(nullptr, L, nullptr, d_U.as<double>(), d_E.as<double>(), d_tab.as<double>(), d_Q.as<int32_t>(),
                             phases ? d_D.as<double>() : nullptr, d_lists.as<int32_t>(), n_q, mu, T, fr.n_w != 0 ? d_W.as<double>() : nullptr,
                             fr.eta, d_part.as<double>(), d_chi.as<double>()));
    TBK_HIP(hipMemcpy(chi_out, d_chi.ptr, out_bytes, hipMemcpyDeviceToHost));
    return TBK_OK;
}

// the whole call: static (fr.n_w = 0, chi_out double [n_q]), dynamic (complex [n_q][n_w]) or orbital-resolved (ob.on, complex [n_q][m][m])
static int chi_whole_call(tbk_model* const* handles, int n_handles, const int32_t* mesh, int mode, double value, double T, int64_t n_q,
                   const int64_t* q, const ChiFreq& fr, const ChiOrb& ob, int matrix_elements, int convention, const double* pos,
                   double* mu_out, double* chi_out) {
    TBK_ARG(mu_out != nullptr, "mu is NULL");
    TBK_ARG(mode == 0 || mode == 1, "mode must be 0 (value = energy) or 1 (value = n_electrons)");
    TBK_ARG(handles != nullptr && n_handles >= 1 && handles[0] != nullptr, "no handles");
    TBK_CHECK(chi_check(T, n_q, q, chi_out, handles[0]->n_orb));
    if (fr.n_w != 0) TBK_CHECK(chi_check_frequencies(fr.n_w, fr.omega, fr.eta, ob.on));
    TBK_CHECK(tbk_eigh_check_arguments(0, convention, pos));
    if (mode == 1)
        TBK_CHECK(tbk_fermi_check_electrons(value, handles[0]->n_orb));
    else
        TBK_ARG(std::isfinite(value), "the energy is not finite");
    // the orbital-resolved call's own arguments, before any device work
    TBK_ARG(matrix_elements != 0 || !ob.on, "the orbital-resolved susceptibility needs the eigenvectors");
    std::vector<int32_t> h_lists;
    TBK_CHECK(chi_orb_lists(ob, handles[0]->n_orb, &h_lists));
    const size_t l_bytes = h_lists.size() * sizeof(int32_t);
    // mu: the slab route of tbk_occupations as it stands
    OccStaged staged;
    TBK_CHECK(staged.make(handles, n_handles, mesh));
    TBK_CHECK(staged.find_mu(mesh, mode, value, mu_out));
    const double mu = mu_out[0];
    const int n_orb = staged.n_orb, dim = staged.dim;
    const int64_t nk = staged.nk_total;
    const bool with_u = matrix_elements != 0, with_d = with_u && convention == 1;
    // (h_lists, h_Q and h_D are the sources of enqueued copies: in front of `res`, whose streams wait before they go)
    std::vector<int32_t> h_Q;
    TBK_CHECK(chi_reduce_q(dim, mesh, n_q, q, &h_Q));
    std::vector<double> h_D;
    if (with_d) TBK_CHECK(mesh_phase_table(dim, mesh, n_orb, n_q, q, pos, &h_D));
    ResidentMesh res;
    TBK_CHECK(res.open(dim, mesh, n_orb, nk));
    // every handle holds the whole mesh's eigensystem and takes a contiguous share of the vectors
    const TetraSlabs share(n_q, n_handles);
    const size_t e_bytes = (size_t)nk * n_orb * sizeof(double);
    // the one place that knows the kind: per vector a double, n_w complex numbers or m x m of them; the frequencies follow the results,
    // the selection the reduced vectors
    const size_t out_per_q = chi_out_per_q(fr, ob);
    const size_t w_bytes = (size_t)fr.n_w * sizeof(double);
    for (int i = 0; i < share.busy(); ++i) {
        tbk_model* m = handles[i];
        const int64_t q_lo = share.lo(i), q_n = share.count(i);
        TBK_CHECK(res.stage(m, CHI_FAMILY, 3 * e_bytes, "the eigenvalues and Fermi tables of the whole mesh", with_u));
        TBK_CHECK(m->ws_mesh_io.reserve((size_t)q_n * (3 * sizeof(int32_t) + out_per_q + (with_d ? n_orb * sizeof(double2) : 0)) + w_bytes + l_bytes + 256));
        // the batch from the memory that is left for the partials, the chunk of the eigenvector walk from what is left then
        size_t free_b = 0, total_b = 0;
        TBK_HIP(hipMemGetInfo(&free_b, &total_b));
        const size_t room = std::max<size_t>(1, std::min(CHI_PART_BUDGET, std::max(m->ws_mesh_work.bytes, free_b / 4)));
        ChiPlan L;
        TBK_CHECK(chi_plan(dim, mesh, nk, n_orb, q_n, fr.n_w, ob.m, ob.tensor, with_u, room, 0, &L));
        TBK_CHECK(m->ws_mesh_work.reserve(L.part_bytes()));
        double* d_E = m->ws_mesh_e.as<double>();
        // ws_mesh_io: the results (and the frequencies of a dynamic call), 256-byte aligned behind them the phases, then the reduced
        // vectors (and the selection of an orbital-resolved call)
        double* d_chi = m->ws_mesh_io.as<double>();
        double* d_W = fr.n_w != 0 ? reinterpret_cast<double*>(m->ws_mesh_io.as<char>() + (size_t)q_n * out_per_q) : nullptr;
        char* behind = m->ws_mesh_io.as<char>() + dos_align256((size_t)q_n * out_per_q + w_bytes);
        double* d_D = with_d ? reinterpret_cast<double*>(behind) : nullptr;
        int32_t* d_Q = reinterpret_cast<int32_t*>(behind + (with_d ? (size_t)q_n * n_orb * sizeof(double2) : 0));
        int32_t* d_lists = d_Q + (size_t)q_n * 3;
        if (l_bytes) TBK_HIP(hipMemcpyAsync(d_lists, h_lists.data(), l_bytes, hipMemcpyHostToDevice, m->stream));
        TBK_CHECK(res.upload(m));
        TBK_HIP(hipMemcpyAsync(d_Q, h_Q.data() + q_lo * 3, (size_t)q_n * 3 * sizeof(int32_t), hipMemcpyHostToDevice, m->stream));
        if (d_W) TBK_HIP(hipMemcpyAsync(d_W, fr.omega, w_bytes, hipMemcpyHostToDevice, m->stream));
        if (with_d)
            TBK_HIP(hipMemcpyAsync(d_D, h_D.data() + (size_t)q_lo * n_orb * 2, (size_t)q_n * n_orb * sizeof(double2), hipMemcpyHostToDevice,
                                   m->stream));
        TBK_CHECK(res.fill(m, with_u));
        TBK_CHECK(chi_launch_all(m->stream, L, res.ev(), m->ws_mesh_u.as<double>(), d_E, d_E + (size_t)nk * n_orb, d_Q, d_D, d_lists, q_n, mu, T,
                                 d_W, fr.eta, m->ws_mesh_work.as<double>(), d_chi));
        TBK_HIP(hipMemcpyAsync(reinterpret_cast<char*>(chi_out) + (size_t)q_lo * out_per_q, d_chi, (size_t)q_n * out_per_q, hipMemcpyDeviceToHost,
                               m->stream));
    }
    // synchronises every handle (the eigensolver's flags are reported as by tbk_eigh) and books the kernel times
    return res.streams.finish(TIMED_CHI);
}

extern "C" int tbk_chi_from_eigensystem(int device, int dim, const int32_t* mesh, int n_orb, const double* E, const double* U, double mu, double T,
                                        int64_t n_q, const int64_t* q, const double* phases, double* chi_out) {
    return chi_from_eigensystem(device, dim, mesh, n_orb, E, U, mu, T, n_q, q, phases, ChiFreq(), ChiOrb(), 0, 0, chi_out);
}

extern "C" int tbk_susceptibility_multi(tbk_model* const* handles, int n_handles, const int32_t* mesh, int mode, double value, double T,
                                        int64_t n_q, const int64_t* q, int matrix_elements, int convention, const double* pos, double* mu_out,
                                        double* chi_out) {
    return chi_whole_call(handles, n_handles, mesh, mode, value, T, n_q, q, ChiFreq(), ChiOrb(), matrix_elements, convention, pos, mu_out, chi_out);
}

extern "C" int tbk_chi_dynamic_plan(int64_t nk, int n_orb, int64_t n_q, int64_t n_w, int matrix_elements, int64_t part_bytes, int64_t* out) {
    TBK_ARG(nk >= 1 && n_orb >= 1 && n_orb <= CHI_MAX_ORB && n_q >= 1 && n_w >= 1 && n_w <= CHI_MAX_NW && part_bytes >= 0 && out != nullptr,
            "nk / n_orb / n_q / n_w < 1, more than 16320 orbitals or 2^23 frequencies, part_bytes < 0 or out is NULL");
    int bt = 0;
    chi_dyn_plan_sizes(nk, n_orb, n_q, n_w, matrix_elements != 0, (size_t)part_bytes, &bt, &out[1], &out[2], &out[3], &out[4], &out[5]);
    out[0] = bt;
    out[6] = CHI_WC;
    return TBK_OK;
}

extern "C" int tbk_chi_dynamic_from_eigensystem(int device, int dim, const int32_t* mesh, int n_orb, const double* E, const double* U, double mu,
                                                double T, int64_t n_q, const int64_t* q, const double* phases, int64_t n_w, const double* omega,
                                                double eta, int64_t part_bytes, double* chi_out) {
    TBK_ARG(part_bytes >= 0, "part_bytes < 0");
    TBK_ARG(n_w >= 1, "n_w < 1");
    return chi_from_eigensystem(device, dim, mesh, n_orb, E, U, mu, T, n_q, q, phases, ChiFreq{n_w, omega, eta}, ChiOrb(), (size_t)part_bytes, 0,
                                chi_out);
}

extern "C" int tbk_dynamic_susceptibility_multi(tbk_model* const* handles, int n_handles, const int32_t* mesh, int mode, double value, double T,
                                                int64_t n_q, const int64_t* q, int64_t n_w, const double* omega, double eta, int matrix_elements,
                                                int convention, const double* pos, double* mu_out, double* chi_out) {
    TBK_ARG(n_w >= 1, "n_w < 1");
    return chi_whole_call(handles, n_handles, mesh, mode, value, T, n_q, q, ChiFreq{n_w, omega, eta}, ChiOrb(), matrix_elements, convention, pos,
                          mu_out, chi_out);
}

extern "C" int tbk_dynamic_susceptibility(tbk_model* m, const int32_t* mesh, int mode, double value, double T, int64_t n_q, const int64_t* q,
                                          int64_t n_w, const double* omega, double eta, int matrix_elements, int convention, const double* pos,
                                          double* mu_out, double* chi_out) {
    return tbk_dynamic_susceptibility_multi(&m, 1, mesh, mode, value, T, n_q, q, n_w, omega, eta, matrix_elements, convention, pos, mu_out, chi_out);
}

extern "C" int tbk_susceptibility(tbk_model* m, const int32_t* mesh, int mode, double value, double T, int64_t n_q, const int64_t* q,
                                  int matrix_elements, int convention, const double* pos, double* mu_out, double* chi_out) {
    return tbk_susceptibility_multi(&m, 1, mesh, mode, value, T, n_q, q, matrix_elements, convention, pos, mu_out, chi_out);
}

extern "C" int tbk_chi_timing(tbk_model* m, double* ms, int64_t* calls, int reset) {
    TBK_ARG(m != nullptr && ms != nullptr && calls != nullptr, "model / ms / calls is NULL");
    return tbk_timed_read(m, TIMED_CHI, 3, ms, calls, nullptr, reset);
}

// ---- the orbital-resolved chi_0[i][j](q) -----------------------------------------------------------------------------------------
extern "C" int tbk_chi_orbital_plan(int64_t nk, int n_orb, int m, int64_t n_q, int64_t part_bytes, int64_t k_slice, int64_t* out) {
    TBK_ARG(nk >= 1 && n_orb >= 1 && n_orb <= CHI_MAX_ORB && m >= 1 && m <= n_orb && n_q >= 1 && part_bytes >= 0 && k_slice >= 0 && out != nullptr,
            "nk / n_orb / m / n_q < 1, more than 16320 orbitals, m > n_orb, part_bytes / k_slice < 0 or out is NULL");
    ChiPlan L;
    chi_orb_plan_sizes(nk, n_orb, m, n_q, (size_t)part_bytes, k_slice, &L);
    out[0] = L.bt;
    out[1] = L.blocks;
    out[2] = L.ks;
    out[3] = L.slices;
    out[4] = L.batch;
    out[5] = L.batches;
    return TBK_OK;
}

extern "C" int tbk_chi_orbital_from_eigensystem(int device, int dim, const int32_t* mesh, int n_orb, const double* E, const double* U, double mu,
                                                double T, int64_t n_q, const int64_t* q, const double* phases, int m, const int32_t* orbitals,
                                                int64_t part_bytes, int64_t k_slice, double* chi_out) {
    TBK_ARG(part_bytes >= 0 && k_slice >= 0, "part_bytes / k_slice < 0");
    return chi_from_eigensystem(device, dim, mesh, n_orb, E, U, mu, T, n_q, q, phases, ChiFreq(), ChiOrb{true, m, orbitals}, (size_t)part_bytes,
                                k_slice, chi_out);
}

extern "C" int tbk_orbital_susceptibility_multi(tbk_model* const* handles, int n_handles, const int32_t* mesh, int mode, double value, double T,
                                                int64_t n_q, const int64_t* q, int m, const int32_t* orbitals, int convention, const double* pos,
                                                double* mu_out, double* chi_out) {
    return chi_whole_call(handles, n_handles, mesh, mode, value, T, n_q, q, ChiFreq(), ChiOrb{true, m, orbitals}, 1, convention, pos, mu_out,
                          chi_out);
}

extern "C" int tbk_orbital_susceptibility(tbk_model* m, const int32_t* mesh, int mode, double value, double T, int64_t n_q, const int64_t* q,
                                          int n_sel, const int32_t* orbitals, int convention, const double* pos, double* mu_out, double* chi_out) {
    return tbk_orbital_susceptibility_multi(&m, 1, mesh, mode, value, T, n_q, q, n_sel, orbitals, convention, pos, mu_out, chi_out);
}

// ---- the four-index chi_0[i][l][j][m](q) -----------------------------------------------------------------------------------------
extern "C" int tbk_chi_tensor_plan(int64_t nk, int n_orb, int m, int64_t n_q, int64_t part_bytes, int64_t k_slice, int64_t* out) {
    TBK_ARG(nk >= 1 && n_orb >= 1 && n_orb <= CHI_MAX_ORB && m >= 1 && m <= n_orb && m <= CHI_TEN_MAX && n_q >= 1 && part_bytes >= 0 &&
                k_slice >= 0 && out != nullptr,
            "nk / n_orb / m / n_q < 1, more than 16320 orbitals, m > n_orb or m > 16, part_bytes / k_slice < 0 or out is NULL");
    ChiPlan L;
    chi_ten_plan_sizes(nk, n_orb, m, n_q, (size_t)part_bytes, k_slice, &L);
    out[0] = L.tr / CHI_TEN_RB;
    out[1] = L.blocks;
    out[2] = L.ks;
    out[3] = L.slices;
    out[4] = L.batch;
    out[5] = L.batches;
    return TBK_OK;
}

extern "C" int tbk_chi_tensor_from_eigensystem(int device, int dim, const int32_t* mesh, int n_orb, const double* E, const double* U, double mu,
                                               double T, int64_t n_q, const int64_t* q, int m, const int32_t* orbitals, int64_t part_bytes,
                                               int64_t k_slice, double* chi_out) {
    TBK_ARG(part_bytes >= 0 && k_slice >= 0, "part_bytes / k_slice < 0");
    return chi_from_eigensystem(device, dim, mesh, n_orb, E, U, mu, T, n_q, q, nullptr, ChiFreq(), ChiOrb{true, m, orbitals, true},
                                (size_t)part_bytes, k_slice, chi_out);
}

extern "C" int tbk_susceptibility_tensor_multi(tbk_model* const* handles, int n_handles, const int32_t* mesh, int mode, double value, double T,
                                               int64_t n_q, const int64_t* q, int m, const int32_t* orbitals, double* mu_out, double* chi_out) {
    return chi_whole_call(handles, n_handles, mesh, mode, value, T, n_q, q, ChiFreq(), ChiOrb{true, m, orbitals, true}, 1, 2, nullptr, mu_out,
                          chi_out);
}

extern "C" int tbk_susceptibility_tensor(tbk_model* m, const int32_t* mesh, int mode, double value, double T, int64_t n_q, const int64_t* q,
                                         int n_sel, const int32_t* orbitals, double* mu_out, double* chi_out) {
    return tbk_susceptibility_tensor_multi(&m, 1, mesh, mode, value, T, n_q, q, n_sel, orbitals, mu_out, chi_out);
}

// ---- the orbital-resolved dynamic chi_0[i][j](q, omega + i eta) -------------------------------------------------------------------
extern "C" int tbk_chi_orbital_dynamic_plan(int64_t nk, int n_orb, int m, int64_t n_q, int64_t n_w, int64_t part_bytes, int64_t k_slice,
                                            int64_t* out) {
    TBK_ARG(nk >= 1 && n_orb >= 1 && n_orb <= CHI_MAX_ORB && m >= 1 && m <= n_orb && n_q >= 1 && n_w >= 1 && n_w <= CHI_ORB_MAX_NW &&
                part_bytes >= 0 && k_slice >= 0 && out != nullptr,
            "nk / n_orb / m / n_q / n_w < 1, more than 16320 orbitals or 65535 frequencies, m > n_orb, part_bytes / k_slice < 0 or out is NULL");
    ChiPlan L;
    chi_orb_dyn_plan_sizes(nk, n_orb, m, n_q, n_w, (size_t)part_bytes, k_slice, &L);
    out[0] = L.bt;
    out[1] = L.blocks;
    out[2] = L.ks;
    out[3] = L.slices;
    out[4] = CHI_OWC;
    out[5] = L.batch;
    out[6] = L.batches;
    out[7] = L.w_pass;
    out[8] = L.passes;
    out[9] = L.batch * L.w_pass;
    return TBK_OK;
}

extern "C" int tbk_chi_orbital_dynamic_from_eigensystem(int device, int dim, const int32_t* mesh, int n_orb, const double* E, const double* U,
                                                        double mu, double T, int64_t n_q, const int64_t* q, const double* phases, int m,
                                                        const int32_t* orbitals, int64_t n_w, const double* omega, double eta,
                                                        int64_t part_bytes, int64_t k_slice, double* chi_out) {
    TBK_ARG(part_bytes >= 0 && k_slice >= 0, "part_bytes / k_slice < 0");
    TBK_ARG(n_w >= 1, "n_w < 1");
    return chi_from_eigensystem(device, dim, mesh, n_orb, E, U, mu, T, n_q, q, phases, ChiFreq{n_w, omega, eta}, ChiOrb{true, m, orbitals},
                                (size_t)part_bytes, k_slice, chi_out);
}

extern "C" int tbk_dynamic_orbital_susceptibility_multi(tbk_model* const* handles, int n_handles, const int32_t* mesh, int mode, double value,
                                                        double T, int64_t n_q, const int64_t* q, int64_t n_w, const double* omega, double eta,
                                                        int m, const int32_t* orbitals, int convention, const double* pos, double* mu_out,
                                                        double* chi_out) {
    TBK_ARG(n_w >= 1, "n_w < 1");
    return chi_whole_call(handles, n_handles, mesh, mode, value, T, n_q, q, ChiFreq{n_w, omega, eta}, ChiOrb{true, m, orbitals}, 1, convention, pos,
                          mu_out, chi_out);
}

extern "C" int tbk_dynamic_orbital_susceptibility(tbk_model* m, const int32_t* mesh, int mode, double value, double T, int64_t n_q,
                                                  const int64_t* q, int64_t n_w, const double* omega, double eta, int n_sel,
                                                  const int32_t* orbitals, int convention, const double* pos, double* mu_out, double* chi_out) {
    return tbk_dynamic_orbital_susceptibility_multi(&m, 1, mesh, mode, value, T, n_q, q, n_w, omega, eta, n_sel, orbitals, convention, pos, mu_out,
                                                    chi_out);
}
