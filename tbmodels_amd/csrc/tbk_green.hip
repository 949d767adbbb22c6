// tbk_green.hip -- the lattice Green's function (the resolvent) of a uniform, periodic k mesh at a list of complex energies.  Not in
// the reference; DESIGN.md section 19 has the quantity, the kernel and the measurements, tools/green_model.py is the statement the
// tests compare with.
//
//   g[k][b](z)    = 1 / (z - E[k][b])                                      E, U of tbk_eigh_device (convention 2), Im z != 0
//   P(k, z)[i][j] = sum_b (g[k][b](z) / NK) U[k][i][b] conj(U[k][j][b])
//   G(R, z)[i][j] = sum_k exp(-2 pi i  num(k, R) / NK) P(k, z)[i][j]       num: the integer phase of tbk_dm.hip
//
// This is the density matrix's transform with a complex weight per energy, and it runs on the density matrix's kernels (tbk_dm.h):
// the phase table of a chunk once, then per TILE of energies one projector launch and one Fourier contraction, whose element axis is
// [energy in tile][n^2]; the partials of every tile stay resident across the chunks and dm_reduce_kernel adds their k slices in
// index order.  The k slices are those of tbk_dm_plan for n^2 elements, whatever the energies: for given (E, U), R, chunk size and
// slab the bits of G(R, z) depend on z alone -- not on the other energies, their order, their number or the tile.
//
//   green_project_kernel  dm_project_kernel's tiling and LDS planes (64 x 64 blocks of one k-point on four waves, 16 x 16 of four
//                         k-points up to 16 orbitals, panels of 16 bands, zeros beyond n) with the planes UNWEIGHTED: Ur, Ui of the
//                         block's rows and of its columns, staged once per panel for all energies of the tile.  Beside them a table
//                         g[energy][band of the panel], made from E and z by the first 16 zt threads of the team.  A lane takes its
//                         A operand (ur, ui) and the B operands of the tile row from LDS once per MFMA step, and per energy forms
//                         a = g (ur + i ui) in registers -- one multiply and one FMA per component -- in front of 4 BT MFMAs:
//                         Gr += ar Ur^T + ai Ui^T, Gi += ai Ur^T - ar Ui^T (the minus is the negate-A bit).  The accumulators of
//                         all energies of the tile live in registers (GREEN_ZT = 4 energies: 256 of them for BT = 4), which is what
//                         bounds the tile.  Output P[table column][energy in tile][n][n].
//
// With a local self-energy Sigma(z) (tools/dyson_model.py) there is no eigensystem to project on:
//
//   P(k, z) = ((z 1 - H(k)) - Sigma(z))^-1 / NK          H(k) of chunk_h (HK_FULL, convention 2)
//
//   green_invert_kernel   one general complex inversion per (k, z), written into the same P layout: Gauss-Jordan in place in LDS
//                         with implicit partial pivoting, panels of 16 pivots, the rank-16 updates on the FP64 matrix pipe; up to 64
//                         orbitals.  Above that (or on request) green_form_kernel, the library's LU and green_scatter_kernel.

#include <algorithm>
#include <cmath>
#include <vector>

#include <rocsolver/rocsolver.h>

#include "tbk_dm.h"

namespace {

typedef double green_d4 __attribute__((ext_vector_type(4)));

constexpr int GREEN_ZT = 4;                              // energies per tile, at most: their accumulators are register-resident
constexpr int64_t GREEN_MAX_Z = 4096;                    // energies per call (include/tbk.h)
constexpr size_t GREEN_P_BUDGET = size_t(1) << 30;       // the projectors of one chunk and one tile
constexpr const char* GREEN_FAMILY = "the Green's function";

// BT tiles of 16 along each side of the workgroup's block of P: 4 (one k-point per workgroup, wave t owns tile row t) or 1 (n <= 16:
// four k-points per workgroup, one per wave).  U, E: of the chunk; z: the tile's zt energies.  Table column j is chunk point j - pad.
template <int BT>
__global__ void __launch_bounds__(DM_THREADS) green_project_kernel(const double2* __restrict__ U, const double* __restrict__ E,
                                                                   const double2* __restrict__ z, int zt, double nk_total, int n, int64_t pad,
                                                                   int64_t nkc, double2* __restrict__ P) {
    constexpr int RB = 16 * BT;                   // rows (and columns) of the block
    constexpr int KPW = BT == 1 ? 4 : 1;          // k-points per workgroup
    constexpr int TEAM = DM_THREADS / KPW;        // threads that stage one k-point's panel
    constexpr int S = BT == 1 ? 18 : 82;          // doubles between the band rows of a plane (tbk_dm.hip)
    __shared__ double planes[KPW][4][16][S];      // Ur, Ui of the block's rows; Ur, Ui of its columns
    __shared__ double2 gtab[KPW][GREEN_ZT][16];   // g / NK of the panel's bands at the tile's energies
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int team = BT == 1 ? wave : 0, tt = tid - team * TEAM;
    const int nb = (n + RB - 1) / RB;
    const int bi = (int)blockIdx.y / nb, bj = (int)blockIdx.y - bi * nb;
    const int64_t j = (int64_t)blockIdx.x * KPW + team;  // table column
    const int64_t k = j - pad;
    const bool valid = k >= 0 && k < nkc;
    const double2* Uk = U + (valid ? (size_t)k * n * n : 0);
    const double* Ek = E + (valid ? (size_t)k * n : 0);
    double(*pl)[16][S] = planes[team];
    double2(*gt)[16] = gtab[team];
    const int ti = BT == 1 ? 0 : wave;  // the wave's tile row
    const bool row_live = bi * RB + ti * 16 < n;  // (wave-uniform)
    green_d4 accr[GREEN_ZT][BT], acci[GREEN_ZT][BT];
#pragma unroll
    for (int zi = 0; zi < GREEN_ZT; ++zi)
#pragma unroll
        for (int tj = 0; tj < BT; ++tj) accr[zi][tj] = acci[zi][tj] = green_d4{0.0, 0.0, 0.0, 0.0};
    const int sb = tt & 15, srow0 = tt >> 4;
    for (int b0 = 0; b0 < n; b0 += 16) {
        __syncthreads();  // the previous panel has been read
        const int b = b0 + sb;
        const bool b_in = valid && b < n;
        if (tt < 16 * zt) {  // (tt >> 4: the energy; 16 zt <= 64 = the smaller team)
            double2 g = make_double2(0.0, 0.0);
            if (b_in) {
                const double2 zz = z[tt >> 4];
                const double dr = zz.x - Ek[b], di = zz.y;
                const double den = (dr * dr + di * di) * nk_total;
                g = make_double2(dr / den, -di / den);
            }
            gt[tt >> 4][sb] = g;
        }
        for (int row = srow0; row < RB; row += TEAM / 16) {
            const int gi = bi * RB + row, gj = bj * RB + row;
            double2 ui = make_double2(0.0, 0.0), uj = ui;
            if (b_in && gi < n) ui = Uk[(size_t)gi * n + b];
            if (bi == bj)
                uj = ui;
            else if (b_in && gj < n)
                uj = Uk[(size_t)gj * n + b];
            pl[0][sb][row] = ui.x;
            pl[1][sb][row] = ui.y;
            pl[2][sb][row] = uj.x;
            pl[3][sb][row] = uj.y;
        }
        __syncthreads();
        if (row_live) {
#pragma unroll 1
            for (int q = 0; q < 4; ++q) {  // (not unrolled, as in dm_project_kernel: the accumulators take the registers)
                const int bq = 4 * q + (lane >> 4);
                const double ur = pl[0][bq][ti * 16 + (lane & 15)], ui = pl[1][bq][ti * 16 + (lane & 15)];
                double br[BT], bim[BT];
#pragma unroll
                for (int tj = 0; tj < BT; ++tj) {
                    br[tj] = pl[2][bq][tj * 16 + (lane & 15)];
                    bim[tj] = pl[3][bq][tj * 16 + (lane & 15)];
                }
#pragma unroll
                for (int zi = 0; zi < GREEN_ZT; ++zi) {
                    if (zi < zt) {  // (uniform)
                        // a = g (ur + i ui), every energy by the same two roundings per component
                        const double2 g = gt[zi][bq];
                        const double ar = __fma_rn(g.x, ur, -__dmul_rn(g.y, ui));
                        const double ai = __fma_rn(g.x, ui, __dmul_rn(g.y, ur));
#pragma unroll
                        for (int tj = 0; tj < BT; ++tj) {
                            if (bj * RB + tj * 16 < n) {  // (uniform)
                                accr[zi][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, br[tj], accr[zi][tj], 0, 0, 0);
                                acci[zi][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, br[tj], acci[zi][tj], 0, 0, 0);
                                accr[zi][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, bim[tj], accr[zi][tj], 0, 0, 0);
                                acci[zi][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, bim[tj], acci[zi][tj], 0, 0, 1);  // - a_r Ui^T
                            }
                        }
                    }
                }
            }
        }
    }
    if (!row_live) return;
    // lane (q, c), register r: row q + 4 r, column c of the tile
#pragma unroll
    for (int zi = 0; zi < GREEN_ZT; ++zi) {
        if (zi >= zt) break;
        double2* Pj = P + ((size_t)j * zt + zi) * n * n;
#pragma unroll
        for (int tj = 0; tj < BT; ++tj) {
            const int gj = bj * RB + tj * 16 + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gi = bi * RB + ti * 16 + (lane >> 4) + 4 * r;
                if (gi < n && gj < n) Pj[(size_t)gi * n + gj] = make_double2(accr[zi][tj][r], acci[zi][tj][r]);
            }
        }
    }
}

// ---- the dressed function: P(k, z) = (z - H(k) - Sigma(z))^-1 / NK by batched inversion ------------------
// Gauss-Jordan in place with implicit partial pivoting, in panels of 16 pivots (tools/dyson_model.py states the same elimination).
// The matrix A = (z 1 - H) - Sigma of one (k, z) is formed in LDS -- two planes (re, im) of NP rows, NP + 1 doubles apart
// -- and stays there; rows never move.  Step j of a panel [j0, j0 + 16):
//     pivot   the row p among those not yet taken with the largest |re| + |im| in column j (ties: the lowest row index; a NaN counts
//             as +inf so that every lane reaches the same row).  Lane = row: every wave of the team finds p by itself.
//     update  of the panel's 16 columns alone (VALU, rank 1): row p becomes a[p][c] / piv (column j: 1 / piv), every other row i
//             a[i][c] - a[i][j] (a[p][c] / piv) (column j: -a[i][j] / piv).
// After its 16 steps the panel's columns hold W = T E, where T is the product of the 16 elementary transformations and E the unit
// columns of the pivot rows: T differs from 1 in those columns alone, so for every OTHER column tile C (the earlier panels, which
// hold columns of the inverse, and the later ones)  T C = mask(C) + W C[pivot rows], mask zeroing the panel's pivot rows: a rank-16
// update, a complex product on v_mfma_f64_16x16x4_f64 (four real MFMAs per complex tile and K step), wave t owning tile row t.  Its
// operands -- W of the tile row, the 16 pivot rows, the tile itself as the accumulator -- go from LDS into registers once, in front
// of a barrier, and the results back behind it.  In the end storage[p_j][c] = inverse[j][p_c]; the store undoes both permutations.
// A pivot of modulus 0 or a non-finite element of the result raises the handle's status word (the smallest (mesh point, energy)
// key wins); no index depends on a value, so a singular input ends like any other.
constexpr int INVERT_PITCH_PAD = 1;  // pitch NP + 1 doubles: 32 consecutive rows of one column lie on 32 different bank pairs
constexpr unsigned long long GREEN_NO_FLAG = ~0ull;

template <int NP>
constexpr size_t invert_lds_bytes() {
    return (size_t)(NP == 16 ? 4 : 1) * ((size_t)2 * NP * (NP + INVERT_PITCH_PAD) * sizeof(double) + (size_t)2 * NP * sizeof(int));
}

// H: [nkc][n][n] of the chunk; z, Sigma: of the tile's zt energies ([zt], [zt][n][n]); table column j is chunk point j - pad, columns
// [0, n_col).  key0: (mesh index of chunk point 0) * GREEN_MAX_Z + index of the tile's first energy, for the status word.
template <int NP>
__global__ void __launch_bounds__(DM_THREADS) green_invert_kernel(const double2* __restrict__ H, const double2* __restrict__ z,
                                                                  const double2* __restrict__ Sigma, int zt, double nk_total, int n, int64_t pad,
                                                                  int64_t nkc, int64_t n_col, unsigned long long key0, double2* __restrict__ P,
                                                                  unsigned long long* __restrict__ flag) {
    constexpr int MPW = NP == 16 ? 4 : 1;     // matrices per workgroup
    constexpr int TEAM = DM_THREADS / MPW;    // threads of one matrix
    constexpr int CG = TEAM / NP;             // column groups of a panel
    constexpr int CPT = 16 / CG;              // panel columns per thread
    constexpr int S = NP + INVERT_PITCH_PAD;  // doubles between two rows of a plane
    constexpr int TR = NP / 16;               // tile rows
    extern __shared__ double invert_lds[];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int team = MPW == 1 ? 0 : wave, tt = tid - team * TEAM;
    double* ar = invert_lds + (size_t)team * (2 * NP * S + NP);  // (2 NP ints = NP doubles)
    double* ai = ar + NP * S;
    int* prow = reinterpret_cast<int*>(ai + NP * S);  // column (step) -> its pivot row
    int* jrow = prow + NP;                            // row -> the step that took it
    const int64_t w = (int64_t)blockIdx.x * MPW + team;
    const bool live = w < n_col * zt;
    const int64_t j = live ? w / zt : 0;
    const int zi = live ? (int)(w - j * zt) : 0;
    const int64_t k = j - pad;
    const bool valid = live && k >= 0 && k < nkc;
    // A = (z 1 - H) - Sigma, zeros beyond n; a column without a mesh point inverts the unit matrix and stores zeros
    {
        const double2 zz = z[zi];
        const double2* Hk = H + (valid ? (size_t)k * n * n : 0);
        const double2* Sz = Sigma + (size_t)zi * n * n;
        for (int e = tt; e < NP * NP; e += TEAM) {
            const int i = e / NP, c = e - i * NP;
            double2 a = make_double2(0.0, 0.0);
            if (i < n && c < n) {
                if (valid) {
                    const double2 h = Hk[(size_t)i * n + c], s = Sz[(size_t)i * n + c];
                    a.x = ((i == c ? zz.x : 0.0) - h.x) - s.x;
                    a.y = ((i == c ? zz.y : 0.0) - h.y) - s.y;
                } else if (i == c) {
                    a.x = 1.0;
                }
            }
            ar[i * S + c] = a.x;
            ai[i * S + c] = a.y;
        }
        if (tt < NP) jrow[tt] = -1;
    }
    const int row = tt & (NP - 1), cg = tt / NP;
    bool used = row >= n, singular = false;
    for (int j0 = 0; j0 < n; j0 += 16) {
        const int jn = n - j0 < 16 ? n - j0 : 16;
        for (int jj = 0; jj < jn; ++jj) {
            const int jc = j0 + jj;
            __syncthreads();  // column jc is up to date
            const double fr = ar[row * S + jc], fi = ai[row * S + jc];
            double best = fabs(fr) + fabs(fi);
            if (!(best >= 0.0)) best = __builtin_inf();
            if (used) best = -1.0;
            int p = row;
#pragma unroll
            for (int off = NP / 2; off > 0; off >>= 1) {
                const double ob = __shfl_xor(best, off, 64);
                const int op = __shfl_xor(p, off, 64);
                if (ob > best || (ob == best && op < p)) {
                    best = ob;
                    p = op;
                }
            }
            // (p is a row below n that no step has taken: at least one is left, and taken rows and padding compare as -1)
            const int src = (lane & ~(NP - 1)) | p;
            const double pr = __shfl(fr, src, 64), pi = __shfl(fi, src, 64);
            singular |= best == 0.0;
            const double den = pr * pr + pi * pi;
            const double ir = pr / den, ii = -pi / den;  // 1 / pivot
            double xr[CPT], xi[CPT], yr[CPT], yi[CPT];
#pragma unroll
            for (int cc = 0; cc < CPT; ++cc) {
                const int c = j0 + cg * CPT + cc;
                xr[cc] = ar[p * S + c];  // (one address per column group: a broadcast)
                xi[cc] = ai[p * S + c];
                yr[cc] = ar[row * S + c];
                yi[cc] = ai[row * S + c];
            }
            __syncthreads();  // every wave has read column jc and row p
#pragma unroll
            for (int cc = 0; cc < CPT; ++cc) {
                const int c = j0 + cg * CPT + cc;
                double tr = ir, ti = ii;  // the new pivot row: a[p][c] / piv, 1 / piv in column jc
                if (c != jc) {
                    tr = xr[cc] * ir - xi[cc] * ii;
                    ti = xr[cc] * ii + xi[cc] * ir;
                }
                double nr = tr, ni = ti;
                if (row != p) {
                    const double mr = fr * tr - fi * ti, mi = fr * ti + fi * tr;
                    nr = c == jc ? -mr : yr[cc] - mr;
                    ni = c == jc ? -mi : yi[cc] - mi;
                }
                ar[row * S + c] = nr;
                ai[row * S + c] = ni;
            }
            if (row == p) {
                used = true;
                if (cg == 0) {
                    prow[jc] = p;
                    jrow[p] = jc;
                }
            }
        }
        if constexpr (TR > 1) {
            // the rank-16 update of the other column tiles
            const int tp = j0 >> 4, q = lane >> 4, c16 = lane & 15;
            const bool busy = wave < TR && wave * 16 < n;  // (wave-uniform; TR <= 4 waves)
            double wr[4], wi[4], br[TR > 1 ? TR - 1 : 1][4], bi[TR > 1 ? TR - 1 : 1][4];
            green_d4 accr[TR > 1 ? TR - 1 : 1], acci[TR > 1 ? TR - 1 : 1];
            __syncthreads();  // the panel's columns are W, its pivot rows are known
            if (busy) {
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    wr[ks] = ar[(wave * 16 + c16) * S + j0 + 4 * ks + q];
                    wi[ks] = ai[(wave * 16 + c16) * S + j0 + 4 * ks + q];
                }
#pragma unroll
                for (int t = 0; t < TR - 1; ++t) {
                    const int tj = t < tp ? t : t + 1;  // (uniform)
#pragma unroll
                    for (int ks = 0; ks < 4; ++ks) {
                        const int kk = 4 * ks + q;
                        const int prw = kk < jn ? prow[j0 + kk] : 0;  // (steps beyond n: no pivot row, a zero operand)
                        br[t][ks] = kk < jn ? ar[prw * S + tj * 16 + c16] : 0.0;
                        bi[t][ks] = kk < jn ? ai[prw * S + tj * 16 + c16] : 0.0;
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int ri = wave * 16 + q + 4 * r;
                        const bool taken = jrow[ri] >= j0;  // a pivot row of this panel starts from zero
                        accr[t][r] = taken ? 0.0 : ar[ri * S + tj * 16 + c16];
                        acci[t][r] = taken ? 0.0 : ai[ri * S + tj * 16 + c16];
                    }
                }
            }
            __syncthreads();  // every operand is in registers
            if (busy) {
#pragma unroll
                for (int t = 0; t < TR - 1; ++t) {
                    const int tj = t < tp ? t : t + 1;
                    if (tj * 16 < n) {  // (uniform: the columns beyond n are zero and stay zero)
#pragma unroll
                        for (int ks = 0; ks < 4; ++ks) {
                            accr[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(wr[ks], br[t][ks], accr[t], 0, 0, 0);
                            acci[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(wr[ks], bi[t][ks], acci[t], 0, 0, 0);
                            accr[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(wi[ks], bi[t][ks], accr[t], 0, 0, 1);  // - w_i b_i
                            acci[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(wi[ks], br[t][ks], acci[t], 0, 0, 0);
                        }
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int ri = wave * 16 + q + 4 * r;
                            ar[ri * S + tj * 16 + c16] = accr[t][r];
                            ai[ri * S + tj * 16 + c16] = acci[t][r];
                        }
                    }
                }
            }
        }
    }
    __syncthreads();
    // inverse[r][s] = storage[prow[r]][jrow[s]], over NK
    if (live) {
        double2* Pj = P + (size_t)w * n * n;
        for (int e = tt; e < n * n; e += TEAM) {
            const int r = e / n, s = e - r * n;
            double2 v = make_double2(0.0, 0.0);
            if (valid) {
                const int at = prow[r] * S + jrow[s];
                v = make_double2(ar[at] / nk_total, ai[at] / nk_total);
                singular |= !(fabs(v.x) <= 1.79769313486231570815e308 && fabs(v.y) <= 1.79769313486231570815e308);
            }
            Pj[e] = v;
        }
        if (valid && singular) atomicMin(flag, key0 + (unsigned long long)k * (unsigned long long)GREEN_MAX_Z + (unsigned long long)zi);
    }
}

// Above the templates, and on request: the library's LU.  A of every (k, z) of the chunk and the tile into a batch workspace,
// [k][energy in tile][n][n] row-major -- which getrf / getri read as the transposes, whose inverses are the transposes of the inverses:
// the buffer ends as the inverses, row-major.
__global__ void __launch_bounds__(256) green_form_kernel(const double2* __restrict__ H, const double2* __restrict__ z, const double2* __restrict__ Sigma,
                                                         int zt, int n, double2* __restrict__ A) {
    const int64_t k = blockIdx.x;
    const int zi = (int)blockIdx.z;
    const size_t nn = (size_t)n * n;
    const double2 zz = z[zi];
    for (size_t e = (size_t)blockIdx.y * 256 + threadIdx.x; e < nn; e += (size_t)gridDim.y * 256) {
        const size_t i = e / n, c = e - i * n;
        const double2 h = H[(size_t)k * nn + e], s = Sigma[(size_t)zi * nn + e];
        A[((size_t)k * zt + zi) * nn + e] = make_double2(((i == c ? zz.x : 0.0) - h.x) - s.x, ((i == c ? zz.y : 0.0) - h.y) - s.y);
    }
}

// P[table column][energy in tile] = A^-1 / NK; the columns in front of the chunk's first point and behind its last are zeros.  info:
// [2][nkc zt] of getrf and getri; a failed member or a non-finite element raises the status word.
__global__ void __launch_bounds__(256) green_scatter_kernel(const double2* __restrict__ A, const int* __restrict__ info, int zt, double nk_total, int n,
                                                            int64_t pad, int64_t nkc, unsigned long long key0, double2* __restrict__ P,
                                                            unsigned long long* __restrict__ flag) {
    const int64_t j = blockIdx.x, k = j - pad;
    const int zi = (int)blockIdx.z;
    const size_t nn = (size_t)n * n;
    const bool valid = k >= 0 && k < nkc;
    bool singular = false;
    if (valid) {
        const int64_t b = k * zt + zi;
        singular = info[b] != 0 || info[nkc * zt + b] != 0;
    }
    for (size_t e = (size_t)blockIdx.y * 256 + threadIdx.x; e < nn; e += (size_t)gridDim.y * 256) {
        double2 v = make_double2(0.0, 0.0);
        if (valid) {
            const double2 a = A[((size_t)k * zt + zi) * nn + e];
            v = make_double2(a.x / nk_total, a.y / nk_total);
            singular |= !(fabs(v.x) <= 1.79769313486231570815e308 && fabs(v.y) <= 1.79769313486231570815e308);
        }
        P[((size_t)j * zt + zi) * nn + e] = v;
    }
    if (singular) atomicMin(flag, key0 + (unsigned long long)k * (unsigned long long)GREEN_MAX_Z + (unsigned long long)zi);
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
// One slab: the density matrix's plan for n^2 elements (its slices are the Green's function's, whatever the energies), the k
// chunk, the energy tile and the tiles of the call.
struct GreenPlan {
    DmPlan D;
    int64_t n_z = 0, zt = 1, tiles = 1, chunk = 1;
    int bt = 4;  // the projector template
    int64_t tile_count(int64_t t) const { return std::min(zt, n_z - t * zt); }
    size_t part_stride() const { return D.with_elements(zt * D.n2).part_bytes(); }  // between the partials of two tiles
    size_t p_bytes() const { return D.with_elements(zt * D.n2).p_bytes(chunk); }
    size_t g_bytes() const { return (size_t)D.n_r * n_z * D.n2 * sizeof(double2); }
    size_t sum_bytes() const { return D.slices > 1 ? D.with_elements(zt * D.n2).rho_bytes() : 0; }  // the sum of one tile's slices
};

// k_chunk > 0: the caller's chunk, and the tile is what keeps its projectors inside the budget; 0: the tile is z_tile (0:
// GREEN_ZT) and the chunk min(auto_chunk, what the budget allows that tile).  The tile does not depend on auto_chunk.
GreenPlan green_plan(const DmPlan& D, int64_t n_z, int64_t z_tile, int64_t k_chunk, int64_t auto_chunk) {
    GreenPlan G;
    G.D = D;
    G.n_z = n_z;
    G.bt = D.n <= 16 ? 1 : 4;
    const int64_t want = std::min<int64_t>(n_z, z_tile > 0 ? std::min<int64_t>(z_tile, GREEN_ZT) : GREEN_ZT);
    const size_t per_point = (size_t)D.n2 * sizeof(double2);  // of one energy
    if (k_chunk > 0) {
        G.chunk = dm_cap_chunk(D, std::min(k_chunk, D.rows));
        const int64_t by_budget = (int64_t)(GREEN_P_BUDGET / (per_point * (size_t)(D.groups(G.chunk) * 4)));
        G.zt = std::max<int64_t>(1, std::min(want, by_budget));
    } else {
        G.zt = want;
        const int64_t by_budget = (int64_t)(GREEN_P_BUDGET / (per_point * (size_t)want)) - 8;
        G.chunk = dm_cap_chunk(D, std::max<int64_t>(4, std::min(std::min(auto_chunk, D.rows), by_budget)));
    }
    G.tiles = (n_z + G.zt - 1) / G.zt;
    return G;
}

int green_check_z(int64_t n_z, const double* z) {
    TBK_ARG(n_z >= 1 && n_z <= GREEN_MAX_Z, "n_z must be 1 to 4096");
    TBK_ARG(z != nullptr, "z is NULL");
    for (int64_t i = 0; i < n_z; ++i) {
        TBK_ARG(std::isfinite(z[2 * i]) && std::isfinite(z[2 * i + 1]), "an energy z is not finite");
        TBK_ARG(z[2 * i + 1] != 0.0, "an energy z has Im z = 0: the resolvent is evaluated off the real axis only");
    }
    return TBK_OK;
}

// The slab's points [c0, c0 + nkc): d_U their eigenvectors, d_E their eigenvalues.  The phase table once, then per tile of energies
// the projectors and their contraction into the tile's partials.  ev (may be NULL): stages 0, 1, 2
int green_launch_chunk(hipStream_t s, const GreenPlan& G, SpanRecorder* ev, const int32_t* d_Rm, const double2* d_z, const double* d_U,
                       const double* d_E, int64_t c0, int64_t nkc, double* d_tab, double2* d_P, char* d_part) {
    const DmPlan& D = G.D;
    const int64_t pad = c0 & 3, ng = (pad + nkc + 3) / 4;
    TBK_CHECK(dm_launch_phase(s, D, ev, d_Rm, c0, nkc, d_tab));
    for (int64_t t = 0; t < G.tiles; ++t) {
        const int zt = (int)G.tile_count(t);
        if (ev) ev->start(1);
        if (G.bt == 1) {
            hipLaunchKernelGGL(green_project_kernel<1>, dim3((unsigned)ng, 1), dim3(DM_THREADS), 0, s, reinterpret_cast<const double2*>(d_U), d_E,
                               d_z + t * G.zt, zt, (double)D.mesh.nk, D.n, pad, nkc, d_P);
        } else {
            const int nb = (D.n + 63) / 64;
            hipLaunchKernelGGL(green_project_kernel<4>, dim3((unsigned)(ng * 4), (unsigned)(nb * nb)), dim3(DM_THREADS), 0, s,
                               reinterpret_cast<const double2*>(d_U), d_E, d_z + t * G.zt, zt, (double)D.mesh.nk, D.n, pad, nkc, d_P);
        }
        if (ev) ev->stop();
        TBK_HIP(hipGetLastError());
        TBK_CHECK(dm_launch_fourier(s, D.with_elements(zt * D.n2), ev, c0, nkc, d_tab, d_P, reinterpret_cast<double2*>(d_part + (size_t)t * G.part_stride())));
    }
    return TBK_OK;
}

// every tile's slices summed (d_sum: the scratch of one tile) and its block of energies put into d_G [n_r][n_z][n^2]
int green_launch_gather(hipStream_t s, const GreenPlan& G, SpanRecorder* ev, const char* d_part, double2* d_sum, double2* d_G) {
    const DmPlan& D = G.D;
    for (int64_t t = 0; t < G.tiles; ++t) {
        const int64_t zt = G.tile_count(t);
        const double2* d_result = nullptr;
        TBK_CHECK(dm_launch_reduce(s, D.with_elements(zt * D.n2), ev, reinterpret_cast<const double2*>(d_part + (size_t)t * G.part_stride()), d_sum,
                                   &d_result));
        const size_t width = (size_t)zt * D.n2 * sizeof(double2);
        TBK_HIP(hipMemcpy2DAsync(d_G + (size_t)t * G.zt * D.n2, (size_t)G.n_z * D.n2 * sizeof(double2), d_result, width, width, (size_t)D.n_r,
                                 hipMemcpyDeviceToDevice, s));
    }
    return TBK_OK;
}

// the vectors and, 256-byte aligned behind them, the energies: one small buffer
size_t green_z_offset(size_t rm_bytes) { return dos_align256(rm_bytes); }

// ---- the dressed function on the host ---------------------------------------------------------------------------------------------
constexpr const char* DYSON_FAMILY = "the dressed Green's function";
constexpr int GREEN_INVERT_MAX = 64;  // orbitals the own inversion kernel takes; above it (or on request) the library's LU

tbk_flag_row green_invert_lds_done;  // green_invert_kernel<64>: more than 64 KiB of dynamic LDS

// what the inversions of one slab read and write beside the plan's buffers
struct DressedWork {
    const double2* d_z = nullptr;       // [n_z]
    const double2* d_sigma = nullptr;   // [n_z][n][n]
    unsigned long long* d_flag = nullptr;
    rocblas_handle blas = nullptr;      // the library route (NULL: the own kernel)
    double2* d_batch = nullptr;         // ... its matrices [chunk][zt][n][n],
    int* d_ipiv = nullptr;              // pivots [chunk][zt][n]
    int* d_info = nullptr;              // and status [2][chunk zt]
    static size_t batch_bytes(const GreenPlan& G) { return dos_align256((size_t)G.chunk * G.zt * G.D.n2 * sizeof(double2)); }
    static size_t ipiv_bytes(const GreenPlan& G) { return dos_align256((size_t)G.chunk * G.zt * G.D.n * sizeof(int)); }
    static size_t library_bytes(const GreenPlan& G) { return batch_bytes(G) + ipiv_bytes(G) + (size_t)2 * G.chunk * G.zt * sizeof(int); }
    void place(const GreenPlan& G, char* base) {
        d_batch = reinterpret_cast<double2*>(base);
        d_ipiv = reinterpret_cast<int*>(base + batch_bytes(G));
        d_info = reinterpret_cast<int*>(base + batch_bytes(G) + ipiv_bytes(G));
    }
};

bool dressed_takes_library(int n_orb, int eigensolver) { return n_orb > GREEN_INVERT_MAX || eigensolver == TBK_EIG_ROCSOLVER; }

int green_check_dressed(int64_t n_z, const double* z, int n_orb, const double* sigma) {
    TBK_ARG(n_z >= 1 && n_z <= GREEN_MAX_Z, "n_z must be 1 to 4096");
    TBK_ARG(z != nullptr && sigma != nullptr, "z / Sigma is NULL");
    for (int64_t i = 0; i < n_z; ++i) TBK_ARG(std::isfinite(z[2 * i]) && std::isfinite(z[2 * i + 1]), "an energy z is not finite");
    const size_t count = (size_t)n_z * n_orb * n_orb * 2;
    for (size_t i = 0; i < count; ++i) TBK_ARG(std::isfinite(sigma[i]), "an element of the self-energy is not finite");
    return TBK_OK;
}

template <int NP>
int green_launch_invert_np(hipStream_t s, const DmPlan& D, const DressedWork& W, const double2* d_H, int64_t t0, int zt, int64_t pad, int64_t nkc,
                           int64_t n_col, unsigned long long key0, double2* d_P) {
    constexpr size_t lds = invert_lds_bytes<NP>();
    if (lds > (size_t(64) << 10)) TBK_HIP(tbk_raise_lds_limit(reinterpret_cast<const void*>(green_invert_kernel<NP>), (int)lds, green_invert_lds_done));
    const int64_t per = NP == 16 ? 4 : 1, blocks = (n_col * zt + per - 1) / per;
    hipLaunchKernelGGL(green_invert_kernel<NP>, dim3((unsigned)blocks), dim3(DM_THREADS), lds, s, d_H, W.d_z + t0, W.d_sigma + (size_t)t0 * D.n2, zt,
                       (double)D.mesh.nk, D.n, pad, nkc, n_col, key0, d_P, W.d_flag);
    return TBK_OK;
}

// The slab's points [c0, c0 + nkc): d_H their H(k), full.  green_launch_chunk with the inversions in the projectors' place
int green_launch_dressed_chunk(hipStream_t s, const GreenPlan& G, SpanRecorder* ev, const int32_t* d_Rm, const DressedWork& W, const double* d_H,
                               int64_t c0, int64_t nkc, double* d_tab, double2* d_P, char* d_part) {
    const DmPlan& D = G.D;
    const int64_t pad = c0 & 3, n_col = (pad + nkc + 3) / 4 * 4;
    const double2* H = reinterpret_cast<const double2*>(d_H);
    TBK_CHECK(dm_launch_phase(s, D, ev, d_Rm, c0, nkc, d_tab));
    for (int64_t t = 0; t < G.tiles; ++t) {
        const int zt = (int)G.tile_count(t);
        const int64_t t0 = t * G.zt;
        const unsigned long long key0 = (unsigned long long)(D.mesh.first + c0) * (unsigned long long)GREEN_MAX_Z + (unsigned long long)t0;
        if (ev) ev->start(1);
        if (W.blas != nullptr) {
            const unsigned gx = (unsigned)std::min<int64_t>(64, (D.n2 + 255) / 256);
            hipLaunchKernelGGL(green_form_kernel, dim3((unsigned)nkc, gx, (unsigned)zt), dim3(256), 0, s, H, W.d_z + t0, W.d_sigma + (size_t)t0 * D.n2, zt,
                               D.n, W.d_batch);
            TBK_HIP(hipGetLastError());
            // (calls stay below 2^29 elements, as those of tbk_eigh)
            const int64_t batch = nkc * zt, step = std::max<int64_t>(1, (int64_t(1) << 29) / D.n2);
            for (int64_t b0 = 0; b0 < batch; b0 += step) {
                const rocblas_int nb = (rocblas_int)std::min(step, batch - b0);
                rocblas_double_complex* A = reinterpret_cast<rocblas_double_complex*>(W.d_batch + (size_t)b0 * D.n2);
                TBK_ROCBLAS(rocsolver_zgetrf_strided_batched(W.blas, D.n, D.n, A, D.n, (rocblas_stride)D.n2, W.d_ipiv + b0 * D.n, (rocblas_stride)D.n,
                                                             W.d_info + b0, nb));
                TBK_ROCBLAS(rocsolver_zgetri_strided_batched(W.blas, D.n, A, D.n, (rocblas_stride)D.n2, W.d_ipiv + b0 * D.n, (rocblas_stride)D.n,
                                                             W.d_info + batch + b0, nb));
            }
            hipLaunchKernelGGL(green_scatter_kernel, dim3((unsigned)n_col, gx, (unsigned)zt), dim3(256), 0, s, W.d_batch, W.d_info, zt, (double)D.mesh.nk,
                               D.n, pad, nkc, key0, d_P, W.d_flag);
        } else if (D.n <= 16) {
            TBK_CHECK(green_launch_invert_np<16>(s, D, W, H, t0, zt, pad, nkc, n_col, key0, d_P));
        } else if (D.n <= 32) {
            TBK_CHECK(green_launch_invert_np<32>(s, D, W, H, t0, zt, pad, nkc, n_col, key0, d_P));
        } else {
            TBK_CHECK(green_launch_invert_np<64>(s, D, W, H, t0, zt, pad, nkc, n_col, key0, d_P));
        }
        if (ev) ev->stop();
        TBK_HIP(hipGetLastError());
        TBK_CHECK(dm_launch_fourier(s, D.with_elements(zt * D.n2), ev, c0, nkc, d_tab, d_P, reinterpret_cast<double2*>(d_part + (size_t)t * G.part_stride())));
    }
    return TBK_OK;
}

// the status word as an error: the first singular (mesh point, energy) of the call
int green_singular_error(int dim, const int32_t* mesh, unsigned long long key, const double* z) {
    if (key == GREEN_NO_FLAG) return TBK_OK;
    int64_t point = (int64_t)(key / (unsigned long long)GREEN_MAX_Z);
    const int64_t zi = (int64_t)(key % (unsigned long long)GREEN_MAX_Z);
    int64_t idx[3] = {0, 0, 0};
    const int64_t index = point;
    for (int d = dim - 1; d >= 0; --d) {
        idx[d] = point % mesh[d];
        point /= mesh[d];
    }
    if (dim == 2)
        tbk_set_error("Singular matrix: z - H(k) - Sigma(z) at mesh point (%lld, %lld) (index %lld) and energy %lld (z = %.17g%+.17gj)", (long long)idx[0],
                      (long long)idx[1], (long long)index, (long long)zi, z[2 * zi], z[2 * zi + 1]);
    else
        tbk_set_error("Singular matrix: z - H(k) - Sigma(z) at mesh point (%lld, %lld, %lld) (index %lld) and energy %lld (z = %.17g%+.17gj)",
                      (long long)idx[0], (long long)idx[1], (long long)idx[2], (long long)index, (long long)zi, z[2 * zi], z[2 * zi + 1]);
    return TBK_ERR_SINGULAR;
}

}  // namespace

extern "C" int tbk_green_dressed_from_matrices(int device, int dim, const int32_t* mesh, int n_orb, const double* H, int64_t k_chunk, int64_t z_tile,
                                               int64_t n_z, const double* z, const double* Sigma, int64_t n_r, const int64_t* R, double* G_out) {
    int64_t nk = 0;
    TBK_CHECK(tetra_check_mesh(dim, mesh, OCC_MESH, &nk));
    TBK_ARG(H != nullptr, "H is NULL");
    TBK_ARG(n_orb >= 1, "n_orb < 1");
    TBK_ARG(k_chunk >= 0 && z_tile >= 0, "k_chunk / z_tile < 0");
    TBK_CHECK(green_check_dressed(n_z, z, n_orb, Sigma));
    TBK_CHECK(dm_check_R(n_r, R, G_out, n_orb));
    TBK_CHECK(tetra_check_device(device));
    DmPlan D;
    TBK_CHECK(dm_plan(dim, mesh, nk, 0, nk, n_orb, n_r, &D));
    const GreenPlan G = green_plan(D, n_z, z_tile, k_chunk, nk);
    std::vector<int32_t> h_Rm;
    TBK_CHECK(dm_reduce_R(dim, mesh, n_r, R, &h_Rm));
    const size_t rm_bytes = h_Rm.size() * sizeof(int32_t), z_bytes = (size_t)n_z * sizeof(double2), s_bytes = (size_t)n_z * D.n2 * sizeof(double2);
    const size_t h_per_k = (size_t)D.n2 * 2;
    DevBuf d_H, d_Rz, d_sigma, d_tab, d_P, d_part, d_G, d_flag, d_lib;
    Owned<rocblas_handle, rocblas_destroy_handle> blas;
    DressedWork W;
    TBK_CHECK(d_part.reserve((size_t)G.tiles * G.part_stride()));
    TBK_CHECK(d_G.reserve(dos_align256(G.g_bytes()) + G.sum_bytes()));
    TBK_CHECK(d_Rz.reserve(green_z_offset(rm_bytes) + z_bytes));
    TBK_CHECK(d_sigma.reserve(s_bytes));
    TBK_CHECK(d_flag.reserve(sizeof(unsigned long long)));
    TBK_CHECK(d_H.reserve((size_t)G.chunk * h_per_k * sizeof(double)));
    TBK_CHECK(d_tab.reserve(D.tab_bytes(G.chunk)));
    TBK_CHECK(d_P.reserve(G.p_bytes()));
    if (dressed_takes_library(n_orb, TBK_EIG_AUTO)) {
        TBK_CHECK(d_lib.reserve(DressedWork::library_bytes(G)));
        TBK_ROCBLAS(rocblas_create_handle(blas.put()));
        W.blas = blas;
        W.place(G, d_lib.as<char>());
    }
    W.d_z = reinterpret_cast<const double2*>(d_Rz.as<char>() + green_z_offset(rm_bytes));
    W.d_sigma = d_sigma.as<double2>();
    W.d_flag = d_flag.as<unsigned long long>();
    double2* d_sum = reinterpret_cast<double2*>(d_G.as<char>() + dos_align256(G.g_bytes()));
    TBK_HIP(hipMemcpy(d_Rz.ptr, h_Rm.data(), rm_bytes, hipMemcpyHostToDevice));
    TBK_HIP(hipMemcpy(d_Rz.as<char>() + green_z_offset(rm_bytes), z, z_bytes, hipMemcpyHostToDevice));
    TBK_HIP(hipMemcpy(d_sigma.ptr, Sigma, s_bytes, hipMemcpyHostToDevice));
    TBK_HIP(hipMemset(d_flag.ptr, 0xff, sizeof(unsigned long long)));
    TBK_HIP(hipMemset(d_part.ptr, 0, (size_t)G.tiles * G.part_stride()));
    for (int64_t c0 = 0; c0 < nk; c0 += G.chunk) {
        const int64_t nkc = std::min(G.chunk, nk - c0);
        TBK_HIP(hipMemcpy(d_H.ptr, H + (size_t)c0 * h_per_k, (size_t)nkc * h_per_k * sizeof(double), hipMemcpyHostToDevice));
        TBK_CHECK(green_launch_dressed_chunk(nullptr, G, nullptr, d_Rz.as<int32_t>(), W, d_H.as<double>(), c0, nkc, d_tab.as<double>(), d_P.as<double2>(),
                                             d_part.as<char>()));
        // (the next chunk's upload overwrites d_H: the null stream orders it behind the kernels)
    }
    TBK_CHECK(green_launch_gather(nullptr, G, nullptr, d_part.as<char>(), d_sum, d_G.as<double2>()));
    unsigned long long key = GREEN_NO_FLAG;
    TBK_HIP(hipMemcpy(&key, d_flag.ptr, sizeof(key), hipMemcpyDeviceToHost));
    TBK_CHECK(green_singular_error(dim, mesh, key, z));
    TBK_HIP(hipMemcpy(G_out, d_G.ptr, G.g_bytes(), hipMemcpyDeviceToHost));
    return TBK_OK;
}

extern "C" int tbk_green_dressed_multi(tbk_model* const* handles, int n_handles, const int32_t* mesh, int64_t n_z, const double* z, const double* Sigma,
                                       int64_t n_r, const int64_t* R, double* G_out) {
    TBK_ARG(handles != nullptr && n_handles >= 1 && handles[0] != nullptr, "no handles");
    TBK_CHECK(green_check_dressed(n_z, z, handles[0]->n_orb, Sigma));
    TBK_CHECK(dm_check_R(n_r, R, G_out, handles[0]->n_orb));
    TetraHandles th;
    TBK_CHECK(th.open(handles, n_handles, mesh, OCC_MESH));
    const int dim = th.dim, n_orb = th.n_orb;
    // (the host buffers the enqueued copies read and write, in front of the streams: they wait before these go)
    std::vector<int32_t> h_Rm;
    std::vector<std::vector<double>> h_k((size_t)th.cut.busy()), partial((size_t)th.cut.busy());  // the slabs' k lists; G of the slabs behind the first
    std::vector<unsigned long long> h_flag((size_t)th.cut.busy(), GREEN_NO_FLAG);                 // the handles' status words
    MeshStreams streams;
    TBK_CHECK(dm_reduce_R(dim, mesh, n_r, R, &h_Rm));
    const size_t rm_bytes = h_Rm.size() * sizeof(int32_t), z_bytes = (size_t)n_z * sizeof(double2);
    const size_t s_off = dos_align256(green_z_offset(rm_bytes) + z_bytes), s_bytes = (size_t)n_z * n_orb * n_orb * sizeof(double2);
    const size_t g_doubles = (size_t)n_r * n_z * n_orb * n_orb * 2;
    for (int i = 0; i < th.cut.busy(); ++i) {  // handles whose slab is empty are skipped
        tbk_model* m = handles[i];  // (locked by th: chunk_h below needs the lock)
        const int64_t nk = th.cut.count(i) * th.plane_pts;
        TBK_CHECK(streams.add(m));
        SpanRecorder* ev = &streams.used.back().ev;
        TBK_CHECK(tbk_dos_mesh_klist(dim, mesh, th.cut.lo(i), th.cut.count(i), &h_k[(size_t)i]));
        DmPlan D;
        TBK_CHECK(dm_plan(dim, mesh, th.nk_total, th.cut.lo(i) * th.plane_pts, nk, n_orb, n_r, &D));
        // G and its partials first: the chunk is chosen from the memory they leave, shared between the chunk's H(k), the inverses of
        // one tile and, on the library route, its batch
        const bool library = dressed_takes_library(n_orb, m->eigensolver);
        GreenPlan G = green_plan(D, n_z, 0, m->k_chunk, nk);
        const size_t part_bytes = (size_t)G.tiles * G.part_stride();
        TBK_CHECK(mesh_reserve(m->ws_dm_part, part_bytes, DYSON_FAMILY, "the partial sums of every energy"));
        TBK_CHECK(mesh_reserve(m->ws_dm_rho, dos_align256(G.g_bytes()) + G.sum_bytes(), DYSON_FAMILY, "G(R, z) of the call"));
        TBK_CHECK(mesh_reserve(m->ws_dm_r, s_off + s_bytes, DYSON_FAMILY, "the self-energy of every energy"));
        TBK_CHECK(m->ws_mesh_k.reserve(h_k[(size_t)i].size() * sizeof(double)));
        TBK_CHECK(m->ws_green_flag.reserve(sizeof(unsigned long long)));
        TBK_HIP(hipMemsetAsync(m->ws_green_flag.ptr, 0xff, sizeof(unsigned long long), m->stream));  // (a call that ended early may have left it raised)
        G = green_plan(D, n_z, 0, m->k_chunk, mesh_eigh_chunk(m, nk, (library ? 2 : 1) * (int)G.zt + 1));
        const int64_t chunk = G.chunk;
        TBK_CHECK(mesh_reserve(m->ws_pdos_u, (size_t)chunk * n_orb * n_orb * sizeof(double2), DYSON_FAMILY, "H(k) of one chunk"));
        TBK_CHECK(m->ws_dm_tab.reserve(D.tab_bytes(chunk)));
        TBK_CHECK(mesh_reserve(m->ws_dm_p, G.p_bytes(), DYSON_FAMILY, "the inverses of one chunk and one energy tile"));
        char* d_rz = m->ws_dm_r.as<char>();
        DressedWork W;
        W.d_z = reinterpret_cast<const double2*>(d_rz + green_z_offset(rm_bytes));
        W.d_sigma = reinterpret_cast<const double2*>(d_rz + s_off);
        W.d_flag = m->ws_green_flag.as<unsigned long long>();
        if (library) {
            TBK_CHECK(mesh_reserve(m->ws_mesh_work, DressedWork::library_bytes(G), DYSON_FAMILY, "the library's batch of one chunk and one energy tile"));
            W.blas = m->blas;
            W.place(G, m->ws_mesh_work.as<char>());
            m->counters[TBK_CNT_LIBRARY_CALLS] += 1;
        }
        double* d_k = m->ws_mesh_k.as<double>();
        TBK_HIP(hipMemcpyAsync(d_k, h_k[(size_t)i].data(), h_k[(size_t)i].size() * sizeof(double), hipMemcpyHostToDevice, m->stream));
        TBK_HIP(hipMemcpyAsync(d_rz, h_Rm.data(), rm_bytes, hipMemcpyHostToDevice, m->stream));
        TBK_HIP(hipMemcpyAsync(d_rz + green_z_offset(rm_bytes), z, z_bytes, hipMemcpyHostToDevice, m->stream));
        TBK_HIP(hipMemcpyAsync(d_rz + s_off, Sigma, s_bytes, hipMemcpyHostToDevice, m->stream));
        TBK_HIP(hipMemsetAsync(m->ws_dm_part.ptr, 0, part_bytes, m->stream));
        double* d_H = m->ws_pdos_u.as<double>();
        const size_t nn2 = (size_t)n_orb * n_orb * 2;
        for (int64_t c0 = 0; c0 < nk; c0 += chunk) {
            const int64_t nkc = std::min(chunk, nk - c0);
            // the FULL H(k) of the chunk, by the routine tbk_eigh_device uses, in pieces of its own choice
            const int64_t piece = choose_chunk(m, nkc, false);
            for (int64_t p0 = 0; p0 < nkc; p0 += piece) {
                const int64_t np = std::min(piece, nkc - p0);
                const tbk_hk_plan_t plan = tbk_hk_plan(m, tbk_staged_operand(m), np, false);
                TBK_CHECK(chunk_h(m, plan, HK_FULL, 2, d_k + (c0 + p0) * dim, nullptr, tbk_one_k_t(), d_H + (size_t)p0 * nn2));
            }
            TBK_CHECK(green_launch_dressed_chunk(m->stream, G, ev, reinterpret_cast<const int32_t*>(d_rz), W, d_H, c0, nkc, m->ws_dm_tab.as<double>(),
                                                 m->ws_dm_p.as<double2>(), m->ws_dm_part.as<char>()));
        }
        double2* d_G = m->ws_dm_rho.as<double2>();
        double2* d_sum = reinterpret_cast<double2*>(m->ws_dm_rho.as<char>() + dos_align256(G.g_bytes()));
        TBK_CHECK(green_launch_gather(m->stream, G, ev, m->ws_dm_part.as<char>(), d_sum, d_G));
        double* h_dst = G_out;
        if (i > 0) {
            try {
                partial[(size_t)i].resize(g_doubles);
            } catch (...) {
                tbk_set_error("cannot allocate the per-handle results");
                return TBK_ERR_MEMORY;
            }
            h_dst = partial[(size_t)i].data();
        }
        TBK_HIP(hipMemcpyAsync(h_dst, d_G, G.g_bytes(), hipMemcpyDeviceToHost, m->stream));
        // the status word comes down with the result and is cleared for the next call
        TBK_HIP(hipMemcpyAsync(&h_flag[(size_t)i], m->ws_green_flag.ptr, sizeof(unsigned long long), hipMemcpyDeviceToHost, m->stream));
        TBK_HIP(hipMemsetAsync(m->ws_green_flag.ptr, 0xff, sizeof(unsigned long long), m->stream));
    }
    // synchronises every handle and books the kernel times; then the status words, the smallest (mesh point, energy) first
    TBK_CHECK(streams.finish(TIMED_DYSON));
    unsigned long long key = GREEN_NO_FLAG;
    for (unsigned long long word : h_flag) key = std::min(key, word);
    TBK_CHECK(green_singular_error(dim, mesh, key, z));
    for (size_t i = 1; i < partial.size(); ++i)  // in handle order
        for (size_t x = 0; x < g_doubles; ++x) G_out[x] += partial[i][x];
    return TBK_OK;
}

extern "C" int tbk_green_dressed(tbk_model* m, const int32_t* mesh, int64_t n_z, const double* z, const double* Sigma, int64_t n_r, const int64_t* R,
                                 double* G_out) {
    return tbk_green_dressed_multi(&m, 1, mesh, n_z, z, Sigma, n_r, R, G_out);
}

extern "C" int tbk_green_dressed_timing(tbk_model* m, double* ms, int64_t* calls, int reset) {
    TBK_ARG(m != nullptr && ms != nullptr && calls != nullptr, "model / ms / calls is NULL");
    return tbk_timed_read(m, TIMED_DYSON, 3, ms, calls, nullptr, reset);
}

extern "C" int tbk_green_plan(int64_t rows, int n_orb, int64_t n_r, int64_t n_z, int64_t z_tile, int64_t k_chunk, int64_t* out) {
    TBK_ARG(rows >= 1 && n_orb >= 1 && n_r >= 1 && out != nullptr, "rows / n_orb / n_r < 1 or out is NULL");
    TBK_ARG(n_z >= 1 && n_z <= GREEN_MAX_Z, "n_z must be 1 to 4096");
    TBK_ARG(z_tile >= 0 && k_chunk >= 0, "z_tile / k_chunk < 0");
    DmPlan D;
    const int32_t line[2] = {1, 1};  // (the slices are a function of rows, n_orb and n_r alone)
    TBK_CHECK(dm_plan(2, line, rows, 0, rows, n_orb, n_r, &D));
    const GreenPlan G = green_plan(D, n_z, z_tile, k_chunk, rows);
    out[0] = D.nr_pad;
    out[1] = D.slices;
    out[2] = D.kps;
    out[3] = G.zt;
    out[4] = G.tiles;
    out[5] = G.chunk;
    out[6] = G.bt;
    return TBK_OK;
}

extern "C" int tbk_green_from_eigensystem(int device, int dim, const int32_t* mesh, int n_orb, const double* E, const double* U, int64_t k_chunk,
                                          int64_t z_tile, int64_t n_z, const double* z, int64_t n_r, const int64_t* R, double* G_out) {
    int64_t nk = 0;
    TBK_CHECK(tetra_check_mesh(dim, mesh, OCC_MESH, &nk));
    TBK_ARG(E != nullptr && U != nullptr, "E / U is NULL");
    TBK_ARG(n_orb >= 1, "n_orb < 1");
    TBK_ARG(k_chunk >= 0 && z_tile >= 0, "k_chunk / z_tile < 0");
    TBK_CHECK(green_check_z(n_z, z));
    TBK_CHECK(dm_check_R(n_r, R, G_out, n_orb));
    TBK_CHECK(tetra_check_device(device));
    DmPlan D;
    TBK_CHECK(dm_plan(dim, mesh, nk, 0, nk, n_orb, n_r, &D));
    const GreenPlan G = green_plan(D, n_z, z_tile, k_chunk, nk);
    std::vector<int32_t> h_Rm;
    TBK_CHECK(dm_reduce_R(dim, mesh, n_r, R, &h_Rm));
    const size_t rm_bytes = h_Rm.size() * sizeof(int32_t), z_bytes = (size_t)n_z * sizeof(double2);
    const size_t e_per_k = (size_t)n_orb, u_per_k = (size_t)n_orb * (size_t)n_orb * 2;
    DevBuf d_E, d_U, d_Rz, d_tab, d_P, d_part, d_G;
    TBK_CHECK(d_part.reserve((size_t)G.tiles * G.part_stride()));
    TBK_CHECK(d_G.reserve(dos_align256(G.g_bytes()) + G.sum_bytes()));
    TBK_CHECK(d_Rz.reserve(green_z_offset(rm_bytes) + z_bytes));
    TBK_CHECK(d_E.reserve((size_t)G.chunk * e_per_k * sizeof(double)));
    TBK_CHECK(d_U.reserve((size_t)G.chunk * u_per_k * sizeof(double)));
    TBK_CHECK(d_tab.reserve(D.tab_bytes(G.chunk)));
    TBK_CHECK(d_P.reserve(G.p_bytes()));
    const double2* d_z = reinterpret_cast<const double2*>(d_Rz.as<char>() + green_z_offset(rm_bytes));
    double2* d_sum = reinterpret_cast<double2*>(d_G.as<char>() + dos_align256(G.g_bytes()));
    TBK_HIP(hipMemcpy(d_Rz.ptr, h_Rm.data(), rm_bytes, hipMemcpyHostToDevice));
    TBK_HIP(hipMemcpy(d_Rz.as<char>() + green_z_offset(rm_bytes), z, z_bytes, hipMemcpyHostToDevice));
    TBK_HIP(hipMemset(d_part.ptr, 0, (size_t)G.tiles * G.part_stride()));
    for (int64_t c0 = 0; c0 < nk; c0 += G.chunk) {
        const int64_t nkc = std::min(G.chunk, nk - c0);
        TBK_HIP(hipMemcpy(d_E.ptr, E + (size_t)c0 * e_per_k, (size_t)nkc * e_per_k * sizeof(double), hipMemcpyHostToDevice));
        TBK_HIP(hipMemcpy(d_U.ptr, U + (size_t)c0 * u_per_k, (size_t)nkc * u_per_k * sizeof(double), hipMemcpyHostToDevice));
        TBK_CHECK(green_launch_chunk(nullptr, G, nullptr, d_Rz.as<int32_t>(), d_z, d_U.as<double>(), d_E.as<double>(), c0, nkc, d_tab.as<double>(),
                                     d_P.as<double2>(), d_part.as<char>()));
    }
    TBK_CHECK(green_launch_gather(nullptr, G, nullptr, d_part.as<char>(), d_sum, d_G.as<double2>()));
    TBK_HIP(hipMemcpy(G_out, d_G.ptr, G.g_bytes(), hipMemcpyDeviceToHost));
    return TBK_OK;
}

extern "C" int tbk_green_function_multi(tbk_model* const* handles, int n_handles, const int32_t* mesh, int64_t n_z, const double* z, int64_t n_r,
                                        const int64_t* R, double* G_out) {
    TBK_CHECK(green_check_z(n_z, z));
    TBK_ARG(handles != nullptr && n_handles >= 1 && handles[0] != nullptr, "no handles");
    TBK_CHECK(dm_check_R(n_r, R, G_out, handles[0]->n_orb));
    TetraHandles th;
    TBK_CHECK(th.open(handles, n_handles, mesh, OCC_MESH));
    const int dim = th.dim, n_orb = th.n_orb;
    // (the host buffers the enqueued copies read and write, in front of the streams: they wait before these go)
    std::vector<int32_t> h_Rm;
    std::vector<std::vector<double>> h_k((size_t)th.cut.busy()), partial((size_t)th.cut.busy());  // the slabs' k lists; G of the slabs behind the first
    MeshStreams streams;
    TBK_CHECK(dm_reduce_R(dim, mesh, n_r, R, &h_Rm));
    const size_t rm_bytes = h_Rm.size() * sizeof(int32_t), z_bytes = (size_t)n_z * sizeof(double2);
    const size_t g_doubles = (size_t)n_r * n_z * n_orb * n_orb * 2;
    for (int i = 0; i < th.cut.busy(); ++i) {  // handles whose slab is empty are skipped
        tbk_model* m = handles[i];
        const int64_t nk = th.cut.count(i) * th.plane_pts;
        TBK_CHECK(streams.add(m));
        SpanRecorder* ev = &streams.used.back().ev;
        TBK_CHECK(tbk_dos_mesh_klist(dim, mesh, th.cut.lo(i), th.cut.count(i), &h_k[(size_t)i]));
        DmPlan D;
        TBK_CHECK(dm_plan(dim, mesh, th.nk_total, th.cut.lo(i) * th.plane_pts, nk, n_orb, n_r, &D));
        // G and its partials first (the tile does not depend on the automatic chunk): the chunk is chosen from the memory they leave,
        // shared between the chunk's eigenvectors and the projectors of one tile
        GreenPlan G = green_plan(D, n_z, 0, m->k_chunk, nk);
        const size_t part_bytes = (size_t)G.tiles * G.part_stride();
        TBK_CHECK(mesh_reserve(m->ws_dm_part, part_bytes, GREEN_FAMILY, "the partial sums of every energy"));
        TBK_CHECK(mesh_reserve(m->ws_dm_rho, dos_align256(G.g_bytes()) + G.sum_bytes(), GREEN_FAMILY, "G(R, z) of the call"));
        TBK_CHECK(m->ws_dm_r.reserve(green_z_offset(rm_bytes) + z_bytes));
        TBK_CHECK(m->ws_mesh_k.reserve(h_k[(size_t)i].size() * sizeof(double)));
        G = green_plan(D, n_z, 0, m->k_chunk, mesh_eigh_chunk(m, nk, 1 + (int)G.zt));
        const int64_t chunk = G.chunk;
        const size_t u_doubles = (size_t)chunk * n_orb * n_orb * 2;
        TBK_CHECK(mesh_reserve(m->ws_pdos_u, (u_doubles + (size_t)chunk * n_orb) * sizeof(double), GREEN_FAMILY, "the eigenvectors of one chunk"));
        TBK_CHECK(m->ws_dm_tab.reserve(D.tab_bytes(chunk)));
        TBK_CHECK(mesh_reserve(m->ws_dm_p, G.p_bytes(), GREEN_FAMILY, "the projectors of one chunk and one energy tile"));
        char* d_rz = m->ws_dm_r.as<char>();
        const double2* d_z = reinterpret_cast<const double2*>(d_rz + green_z_offset(rm_bytes));
        double* d_k = m->ws_mesh_k.as<double>();
        TBK_HIP(hipMemcpyAsync(d_k, h_k[(size_t)i].data(), h_k[(size_t)i].size() * sizeof(double), hipMemcpyHostToDevice, m->stream));
        TBK_HIP(hipMemcpyAsync(d_rz, h_Rm.data(), rm_bytes, hipMemcpyHostToDevice, m->stream));
        TBK_HIP(hipMemcpyAsync(d_rz + green_z_offset(rm_bytes), z, z_bytes, hipMemcpyHostToDevice, m->stream));
        TBK_HIP(hipMemsetAsync(m->ws_dm_part.ptr, 0, part_bytes, m->stream));
        double* d_U = m->ws_pdos_u.as<double>();
        double* d_E = d_U + u_doubles;
        for (int64_t c0 = 0; c0 < nk; c0 += chunk) {
            const int64_t nkc = std::min(chunk, nk - c0);
            TBK_CHECK(tbk_eigh_device(m, d_k + c0 * dim, nkc, 2, nullptr, d_E, d_U));
            TBK_CHECK(green_launch_chunk(m->stream, G, ev, reinterpret_cast<const int32_t*>(d_rz), d_z, d_U, d_E, c0, nkc, m->ws_dm_tab.as<double>(),
                                         m->ws_dm_p.as<double2>(), m->ws_dm_part.as<char>()));
        }
        double2* d_G = m->ws_dm_rho.as<double2>();
        double2* d_sum = reinterpret_cast<double2*>(m->ws_dm_rho.as<char>() + dos_align256(G.g_bytes()));
        TBK_CHECK(green_launch_gather(m->stream, G, ev, m->ws_dm_part.as<char>(), d_sum, d_G));
        double* h_dst = G_out;
        if (i > 0) {
            try {
                partial[(size_t)i].resize(g_doubles);
            } catch (...) {
                tbk_set_error("cannot allocate the per-handle results");
                return TBK_ERR_MEMORY;
            }
            h_dst = partial[(size_t)i].data();
        }
        TBK_HIP(hipMemcpyAsync(h_dst, d_G, G.g_bytes(), hipMemcpyDeviceToHost, m->stream));
    }
    // synchronises every handle (the eigenvector flags are reported as by tbk_eigh) and books the kernel times
    TBK_CHECK(streams.finish(TIMED_GREEN));
    for (size_t i = 1; i < partial.size(); ++i)  // in handle order
        for (size_t x = 0; x < g_doubles; ++x) G_out[x] += partial[i][x];
    return TBK_OK;
}

extern "C" int tbk_green_function(tbk_model* m, const int32_t* mesh, int64_t n_z, const double* z, int64_t n_r, const int64_t* R, double* G_out) {
    return tbk_green_function_multi(&m, 1, mesh, n_z, z, n_r, R, G_out);
}

extern "C" int tbk_green_timing(tbk_model* m, double* ms, int64_t* calls, int reset) {
    TBK_ARG(m != nullptr && ms != nullptr && calls != nullptr, "model / ms / calls is NULL");
    return tbk_timed_read(m, TIMED_GREEN, 3, ms, calls, nullptr, reset);
}
