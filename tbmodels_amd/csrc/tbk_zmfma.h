// tbk_zmfma.h -- the blocks of complex FP64 arithmetic on v_mfma_f64_16x16x4_f64 that more than one family uses (DESIGN.md section
// 28): the vector type, the complex MFMA step in its three forms, the geometry of a staged panel of 16, the overlap panel of
// tbk_chi.hip and tbk_berry.hip, the store of a wave's tiles, and the Gauss-Jordan elimination of tbk_green.hip and tbk_surface.h.
// Device code only, in an unnamed namespace: each translation unit instantiates its own.  Matrices are staged as planes (Re, Im) of
// doubles in LDS; an operand of the instruction is one double per lane, lane (q = lane / 16, c = lane % 16) feeding A[c][k + q] and
// B[k + q][c] of a K step of four and holding C[q + 4 r][c] in register r = 0 ... 3 of the accumulator.
#pragma once

#include <cfloat>  // DBL_MAX: the one bound of the "is it finite" tests

#include "tbk_internal.h"

namespace {

typedef double zd4 __attribute__((ext_vector_type(4)));

// ---- the complex step: four real MFMAs on the accumulators (cr, ci) of one tile ------------------------------------------------------
// The minus sign of each form is the instruction's negate bit (the last argument), always on the A slot: no operand is negated on the
// vector unit.  The order of the two updates of each accumulator is part of a result's bits; the call sites rely on it.
//   zmfma_ab    C += A B       cr += ar br - ai bi,  ci += ar bi + ai br     (the plane products; zgj_invert's rank-16 update writes it out)
//   zmfma_ahb   C += A^H B     cr += ar br + ai bi,  ci += ar bi - ai br     (A given by its rows: the overlaps, the Fourier step)
//   zmfma_abh   C += A B^H     cr += ar br + ai bi,  ci += ai br - ar bi     (B given by its rows: the projectors)
__device__ __forceinline__ void zmfma_ab(double ar, double ai, double br, double bi, zd4& cr, zd4& ci) {
    cr = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, br, cr, 0, 0, 0);
    ci = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, bi, ci, 0, 0, 0);
    cr = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, bi, cr, 0, 0, 1);
    ci = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, br, ci, 0, 0, 0);
}

__device__ __forceinline__ void zmfma_ahb(double ar, double ai, double br, double bi, zd4& cr, zd4& ci) {
    cr = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, br, cr, 0, 0, 0);
    cr = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, bi, cr, 0, 0, 0);
    ci = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, bi, ci, 0, 0, 0);
    ci = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, br, ci, 0, 0, 1);
}

__device__ __forceinline__ void zmfma_abh(double ar, double ai, double br, double bi, zd4& cr, zd4& ci) {
    cr = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, br, cr, 0, 0, 0);
    cr = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, bi, cr, 0, 0, 0);
    ci = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, br, ci, 0, 0, 0);
    ci = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, bi, ci, 0, 0, 1);
}

// ---- a staged panel: the geometry of dm_project_kernel, green_project_kernel, chi_overlap_kernel, chi_orbital_kernel and
// berry_link_kernel -----------------------------------------------------------------------------------------------------------------
// A workgroup of 256 threads owns a block of RB x RB elements, BT tiles of 16 along each side: BT = 4, one item (a k-point, a link, a
// slice) per workgroup and wave t on tile row t, or BT = 1 (up to 16 rows), four items per workgroup and one per wave.  The
// contraction index goes through LDS in panels of 16, four planes [16][S] per item: (Re, Im) of the A side and of the B side, a row
// per contraction index, zeros beyond the matrix.  S = 18 or 82 doubles between the rows: the 16 rows a wave stores at once (a
// thread per contraction index) land in 16 different bank pairs, the four rows a wave reads at once for an operand (nearly) so; a
// wave that stores along a row has no conflict at any pitch.  Every K step of the panel is then one ds_read_b64 per lane and operand.
// The loop over the four K steps of a panel is not unrolled in any of the kernels: with the operands of all four steps at once
// dm_project_kernel<4> takes 344 registers, 96 of them accumulators.
template <int BT>
struct ZPanel {
    static constexpr int THREADS = 256;
    static constexpr int RB = 16 * BT;           // rows (and columns) of the block
    static constexpr int KPW = BT == 1 ? 4 : 1;  // items per workgroup
    static constexpr int TEAM = THREADS / KPW;   // threads that stage one item's panel
    static constexpr int S = BT == 1 ? 18 : 82;  // doubles between the rows of a plane
};

// M = A^H (D B) over the rows [0, n) of A and B, for the wave's tile row ti of block (bi, bj): the whole panel loop.  A, B: row-major
// with pitch n, of which the columns [0, m) count (the caller has added its column offset); Dv: NULL or a factor per row, applied
// while staging.  pl: the team's four planes [4][16][S], as doubles.  Per panel of 16 rows: a barrier, the team's threads stage Re, Im of A's columns of block bi and of D B's of block bj
// (zeros beyond n, beyond m and without `valid`), a barrier, and four K steps of zmfma_ahb on the BT tiles (those beyond m skipped,
// wave-uniform).  tt: the thread in its team.  Two barriers per panel, which every thread of the workgroup must reach.  Stores and K
// steps address the planes from one pointer into plane 0 plus multiples of PLANE: with an index computed per plane
// berry_link_kernel<4, true> takes four registers more.
template <int BT>
__device__ __forceinline__ void zpanel_overlap(const double2* A, const double2* B, const double2* Dv, bool valid, int n, int m, int bi, int bj,
                                               double* pl, int tt, int ti, int lane, bool row_live, zd4 (&accr)[BT],
                                               zd4 (&acci)[BT]) {
    constexpr int RB = ZPanel<BT>::RB, TEAM = ZPanel<BT>::TEAM, S = ZPanel<BT>::S, PLANE = 16 * S;
#pragma unroll
    for (int tj = 0; tj < BT; ++tj) accr[tj] = acci[tj] = zd4{0.0, 0.0, 0.0, 0.0};
    const int sc = tt % RB, so0 = tt / RB;  // the column of the panel and the first row this thread stages
    const int col_a = bi * RB + sc, col_b = bj * RB + sc;
    for (int i0 = 0; i0 < n; i0 += 16) {
        __syncthreads();  // the previous panel has been read
#pragma unroll
        for (int o = so0; o < 16; o += TEAM / RB) {
            const int i = i0 + o;
            const bool i_in = valid && i < n;
            double2 ua = make_double2(0.0, 0.0), ub = ua;
            if (i_in && col_a < m) ua = A[(size_t)i * n + col_a];
            if (i_in && col_b < m) {
                ub = B[(size_t)i * n + col_b];
                if (Dv) {
                    const double2 d = Dv[i];
                    ub = make_double2(d.x * ub.x - d.y * ub.y, d.x * ub.y + d.y * ub.x);
                }
            }
            double* st = pl + o * S + sc;  // row o, column sc of plane 0; the planes are PLANE apart
            st[0] = ua.x;
            st[PLANE] = ua.y;
            st[2 * PLANE] = ub.x;
            st[3 * PLANE] = ub.y;
        }
        __syncthreads();
        if (row_live) {
#pragma unroll 1
            for (int q4 = 0; q4 < 4; ++q4) {  // (not unrolled: ZPanel's note on registers)
                const double* at = pl + (4 * q4 + (lane >> 4)) * S + (lane & 15);  // the lane's row of plane 0; the planes are PLANE apart
                const double ar = at[ti * 16], ai = at[PLANE + ti * 16];
#pragma unroll
                for (int tj = 0; tj < BT; ++tj) {
                    if (bj * RB + tj * 16 < m) {  // (uniform)
                        const double br = at[2 * PLANE + tj * 16], bim = at[3 * PLANE + tj * 16];
                        zmfma_ahb(ar, ai, br, bim, accr[tj], acci[tj]);
                    }
                }
            }
        }
    }
}

// The wave's BT tiles, whose first element is (row0, col0), into a row-major complex n x n matrix; rows and columns beyond n are not
// written.  Lane (q, c), register r: row q + 4 r, column c of a tile.
template <int BT>
__device__ __forceinline__ void ztiles_store(double2* out, int n, int row0, int col0, int lane, const zd4 (&cr)[BT], const zd4 (&ci)[BT]) {
#pragma unroll
    for (int tj = 0; tj < BT; ++tj) {
        const int col = col0 + tj * 16 + (lane & 15);
        if (col < n) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = row0 + (lane >> 4) + 4 * r;
                if (row < n) out[(size_t)row * n + col] = make_double2(cr[tj][r], ci[tj][r]);
            }
        }
    }
}

// ---- the inversion of one complex matrix in LDS (tools/dyson_model.py states the same elimination) --------------------
// Gauss-Jordan in place with implicit partial pivoting, in panels of 16 pivots.  The matrix lies in two planes (re, im) of NP rows,
// NP + 1 doubles apart (32 consecutive rows of one column lie on 32 different bank pairs), and stays there; rows never move.
// THREADS threads work on it, tid among them; n rows and columns count, the rest is zero.  Step j of a panel [j0, j0 + 16):
//     pivot   the row p among those not yet taken with the largest |re| + |im| in column j (ties: the lowest row index; a NaN counts
//             as +inf so that every lane reaches the same row).  Lane = row: every wave finds p by itself.
//     update  of the panel's 16 columns alone (VALU, rank 1): row p becomes a[p][c] / piv (column j: 1 / piv), every other row i
//             a[i][c] - a[i][j] (a[p][c] / piv) (column j: -a[i][j] / piv).
// After its 16 steps the panel's columns hold W = T E, where T is the product of the 16 elementary transformations and E the unit
// columns of the pivot rows: T differs from 1 in those columns alone, so for every OTHER column tile C (the earlier panels, which
// hold columns of the inverse, and the later ones)  T C = mask(C) + W C[pivot rows], mask zeroing the panel's pivot rows: a rank-16
// update (zmfma_ab's four products), wave t owning tile row t.  Its operands -- W of the tile row, the 16 pivot rows, the tile itself as the
// accumulator -- go from LDS into registers once, in front of a barrier, and the results back behind it.  No index depends on a
// value, so a singular input ends like any other.
// jrow must be -1 and the planes written before the call (its first barrier orders them); afterwards, behind a barrier of the
// caller's, inverse[r][s] = storage[prow[r]][jrow[s]].  Returns whether a pivot was exactly zero (the same value on every thread).
template <int NP, int THREADS>
__device__ __forceinline__ bool zgj_invert(double* ar, double* ai, int* prow, int* jrow, int n, int tid) {
    constexpr int CG = THREADS / NP;  // column groups of a panel
    constexpr int CPT = 16 / CG;      // panel columns per thread
    constexpr int S = NP + 1;
    constexpr int TR = NP / 16;
    const int lane = tid & 63, wave = tid >> 6;
    const int row = tid & (NP - 1), cg = tid / NP;
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
            // the rank-16 update of the other column tiles: T C = mask(C) + W C[pivot rows]
            const int tp = j0 >> 4, q = lane >> 4, c16 = lane & 15;
            const bool busy = wave < TR && wave * 16 < n;  // (wave-uniform)
            double wr[4], wi[4], br[TR - 1][4], bi[TR - 1][4];
            zd4 accr[TR - 1], acci[TR - 1];
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
                            // zmfma_ab, written out: through the call the NP = 32 kernels of the layered families are built in
                            // another order and transmission_kernel<32> measured 0.5 % slower (DESIGN_LOG R29.1)
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
    return singular;
}

}  // namespace
