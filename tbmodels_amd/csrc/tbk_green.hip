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

#include "tbk_lattice.h"
#include "tbk_zmfma.h"

namespace {


// BT tiles of 16 along each side of the workgroup's block of P: 4 (one k-point per workgroup, wave t owns tile row t) or 1 (n <= 16:
// four k-points per workgroup, one per wave).  U, E: of the chunk; z: the tile's zt energies.  Table column j is chunk point j - pad.
template <int BT>
__global__ void __launch_bounds__(DM_THREADS) green_project_kernel(const double2* __restrict__ U, const double* __restrict__ E,
                                                                   const double2* __restrict__ z, int zt, double nk_total, int n, int64_t pad,
                                                                   int64_t nkc, double2* __restrict__ P) {
    using Geo = ZPanel<BT>;  // (tbk_zmfma.h; an item is a k-point)
    constexpr int RB = Geo::RB, KPW = Geo::KPW, TEAM = Geo::TEAM, S = Geo::S;
    static_assert(DM_THREADS == Geo::THREADS, "the panel's workgroup");
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
    zd4 accr[GREEN_ZT][BT], acci[GREEN_ZT][BT];
#pragma unroll
    for (int zi = 0; zi < GREEN_ZT; ++zi)
#pragma unroll
        for (int tj = 0; tj < BT; ++tj) accr[zi][tj] = acci[zi][tj] = zd4{0.0, 0.0, 0.0, 0.0};
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
            for (int q = 0; q < 4; ++q) {  // (not unrolled: ZPanel's note on registers)
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
                                // zmfma_abh's four products with the two accumulators taken in turn, Gr Gi Gr Gi: this site's own
                                // copy.  With GREEN_ZT x BT accumulator pairs in flight the shared step's order (Gr Gr Gi Gi)
                                // measured 0.2 - 0.4 % slower at 64 energies (DESIGN_LOG R29.1); each accumulator's own order,
                                // and so the bits, are the step's
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
    // lane (q, c), register r: row q + 4 r, column c of the tile (ztiles_store's loop, kept here with the kernel's own MFMA order:
    // the kernel's built code is then what it was measured as)
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
// The matrix A = (z 1 - H) - Sigma of one (k, z) is formed in LDS -- two planes (re, im) of NP rows, NP + 1 doubles apart -- and
// inverted there by zgj_invert (tbk_zmfma.h: Gauss-Jordan with implicit partial pivoting, panels of 16 pivots, the rank-16 updates on
// the matrix pipe), which leaves storage[p_j][c] = inverse[j][p_c]; the store undoes both permutations.  A pivot of modulus 0 or a
// non-finite element of the result raises the handle's status word (the smallest (mesh point, energy) key wins).
template <int NP>
constexpr size_t invert_lds_bytes() {
    return (size_t)(NP == 16 ? 4 : 1) * ((size_t)2 * NP * (NP + 1) * sizeof(double) + (size_t)2 * NP * sizeof(int));
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
    constexpr int S = NP + 1;                 // doubles between two rows of a plane (zgj_invert's)
    extern __shared__ double invert_lds[];
    const int tid = (int)threadIdx.x, wave = tid >> 6;
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
    bool singular = zgj_invert<NP, TEAM>(ar, ai, prow, jrow, n, tt);
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
                singular |= !(fabs(v.x) <= DBL_MAX && fabs(v.y) <= DBL_MAX);
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
            singular |= !(fabs(v.x) <= DBL_MAX && fabs(v.y) <= DBL_MAX);
        }
        P[((size_t)j * zt + zi) * nn + e] = v;
    }
    if (singular) atomicMin(flag, key0 + (unsigned long long)k * (unsigned long long)GREEN_MAX_Z + (unsigned long long)zi);
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
int green_check_z(int64_t n_z, const double* z) {
    TBK_ARG(n_z >= 1 && n_z <= GREEN_MAX_Z, "n_z must be 1 to 4096");
    TBK_ARG(z != nullptr, "z is NULL");
    for (int64_t i = 0; i < n_z; ++i) {
        TBK_ARG(std::isfinite(z[2 * i]) && std::isfinite(z[2 * i + 1]), "an energy z is not finite");
        TBK_ARG(z[2 * i + 1] != 0.0, "an energy z has Im z = 0: the resolvent is evaluated off the real axis only");
    }
    return TBK_OK;
}

// The Green's function as the drivers of tbk_lattice.h see it: per tile of energies the projectors from the chunk's eigensystem.
struct GreenFamily : LatticeFamily {
    GreenFamily(int64_t n_z_, const double* z_) : LatticeFamily(TIMED_GREEN, n_z_, z_) {
        family = "the Green's function";
        part_what = "the partial sums of every energy";
        result_what = "G(R, z) of the call";
        in_what = "the eigenvectors of one chunk";
        p_what = "the projectors of one chunk and one energy tile";
    }
    int share(int zt, bool) const override { return 1 + zt; }  // the chunk's eigenvectors and the projectors of one tile
    int fill_p(const LatticeChunk& c, int64_t t) const override {
        const GreenPlan& G = c.G;
        const DmPlan& D = G.D;
        const int zt = (int)G.tile_count(t);
        const double2* U = reinterpret_cast<const double2*>(c.d_in);
        if (G.bt == 1)
            hipLaunchKernelGGL(green_project_kernel<1>, c.project_grid(), dim3(DM_THREADS), 0, c.s, U, c.d_E(), c.d_z + t * G.zt, zt, (double)D.mesh.nk, D.n,
                               c.pad, c.nkc, c.d_P);
        else
            hipLaunchKernelGGL(green_project_kernel<4>, c.project_grid(), dim3(DM_THREADS), 0, c.s, U, c.d_E(), c.d_z + t * G.zt, zt, (double)D.mesh.nk, D.n,
                               c.pad, c.nkc, c.d_P);
        return TBK_OK;
    }
};

// ---- the dressed function on the host ---------------------------------------------------------------------------------------------
constexpr int GREEN_INVERT_MAX = 64;  // orbitals the own inversion kernel takes; above it (or on request) the library's LU

tbk_flag_row green_invert_lds_done;  // green_invert_kernel<64>: more than 64 KiB of dynamic LDS

int green_check_dressed(int64_t n_z, const double* z, int n_orb, const double* sigma) {
    TBK_ARG(n_z >= 1 && n_z <= GREEN_MAX_Z, "n_z must be 1 to 4096");
    TBK_ARG(z != nullptr && sigma != nullptr, "z / Sigma is NULL");
    for (int64_t i = 0; i < n_z; ++i) TBK_ARG(std::isfinite(z[2 * i]) && std::isfinite(z[2 * i + 1]), "an energy z is not finite");
    const size_t count = (size_t)n_z * n_orb * n_orb * 2;
    for (size_t i = 0; i < count; ++i) TBK_ARG(std::isfinite(sigma[i]), "an element of the self-energy is not finite");
    return TBK_OK;
}

// key0: (mesh index of chunk point 0) * GREEN_MAX_Z + index of the tile's first energy t0
template <int NP>
int green_launch_invert_np(const LatticeChunk& c, int64_t t0, int zt, int64_t n_col, unsigned long long key0) {
    const DmPlan& D = c.G.D;
    constexpr size_t lds = invert_lds_bytes<NP>();
    if (lds > (size_t(64) << 10)) TBK_HIP(tbk_raise_lds_limit(reinterpret_cast<const void*>(green_invert_kernel<NP>), (int)lds, green_invert_lds_done));
    const int64_t per = NP == 16 ? 4 : 1, blocks = (n_col * zt + per - 1) / per;
    hipLaunchKernelGGL(green_invert_kernel<NP>, dim3((unsigned)blocks), dim3(DM_THREADS), lds, c.s, reinterpret_cast<const double2*>(c.d_in), c.d_z + t0,
                       c.d_sigma + (size_t)t0 * D.n2, zt, (double)D.mesh.nk, D.n, c.pad, c.nkc, n_col, key0, c.d_P, c.d_flag);
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

// The dressed function: per tile of energies the inverses from the chunk's full H(k), by the own kernel or the library's LU, whose
// batch [chunk][zt][n][n], pivots [chunk][zt][n] and status [2][chunk zt] are the route's workspace.
struct DressedFamily : LatticeFamily {
    DressedFamily(int64_t n_z_, const double* z_, const double* sigma_) : LatticeFamily(TIMED_DYSON, n_z_, z_, sigma_) {
        family = "the dressed Green's function";
        part_what = "the partial sums of every energy";
        result_what = "G(R, z) of the call";
        const_what = "the self-energy of every energy";
        in_what = "H(k) of one chunk";
        p_what = "the inverses of one chunk and one energy tile";
        work_what = "the library's batch of one chunk and one energy tile";
        needs_h = true;
        has_status = true;
    }
    static size_t batch_bytes(const GreenPlan& G) { return dos_align256((size_t)G.chunk * G.zt * G.D.n2 * sizeof(double2)); }
    static size_t ipiv_bytes(const GreenPlan& G) { return dos_align256((size_t)G.chunk * G.zt * G.D.n * sizeof(int)); }
    // the chunk's H(k), the inverses of one tile and, on the library route, its batch
    int share(int zt, bool library) const override { return (library ? 2 : 1) * zt + 1; }
    bool library(int n_orb, int eigensolver) const override { return n_orb > GREEN_INVERT_MAX || eigensolver == TBK_EIG_ROCSOLVER; }
    size_t work_bytes(const GreenPlan& G) const override { return batch_bytes(G) + ipiv_bytes(G) + (size_t)2 * G.chunk * G.zt * sizeof(int); }
    int status_error(unsigned long long word) const override { return green_singular_error(dim, mesh, word, z); }
    int fill_p(const LatticeChunk& c, int64_t t) const override {
        const GreenPlan& G = c.G;
        const DmPlan& D = G.D;
        const int zt = (int)G.tile_count(t);
        const int64_t t0 = t * G.zt, n_col = c.ng * 4;
        const unsigned long long key0 = (unsigned long long)(D.mesh.first + c.c0) * (unsigned long long)GREEN_MAX_Z + (unsigned long long)t0;
        if (c.blas != nullptr) {
            double2* d_batch = reinterpret_cast<double2*>(c.d_work);
            int* d_ipiv = reinterpret_cast<int*>(c.d_work + batch_bytes(G));
            int* d_info = reinterpret_cast<int*>(c.d_work + batch_bytes(G) + ipiv_bytes(G));
            const unsigned gx = (unsigned)std::min<int64_t>(64, (D.n2 + 255) / 256);
            hipLaunchKernelGGL(green_form_kernel, dim3((unsigned)c.nkc, gx, (unsigned)zt), dim3(256), 0, c.s, reinterpret_cast<const double2*>(c.d_in),
                               c.d_z + t0, c.d_sigma + (size_t)t0 * D.n2, zt, D.n, d_batch);
            TBK_HIP(hipGetLastError());
            // (calls stay below 2^29 elements, as those of tbk_eigh)
            const int64_t batch = c.nkc * zt, step = std::max<int64_t>(1, (int64_t(1) << 29) / D.n2);
            for (int64_t b0 = 0; b0 < batch; b0 += step) {
                const rocblas_int nb = (rocblas_int)std::min(step, batch - b0);
                rocblas_double_complex* A = reinterpret_cast<rocblas_double_complex*>(d_batch + (size_t)b0 * D.n2);
                TBK_ROCBLAS(rocsolver_zgetrf_strided_batched(c.blas, D.n, D.n, A, D.n, (rocblas_stride)D.n2, d_ipiv + b0 * D.n, (rocblas_stride)D.n,
                                                             d_info + b0, nb));
                TBK_ROCBLAS(rocsolver_zgetri_strided_batched(c.blas, D.n, A, D.n, (rocblas_stride)D.n2, d_ipiv + b0 * D.n, (rocblas_stride)D.n,
                                                             d_info + batch + b0, nb));
            }
            hipLaunchKernelGGL(green_scatter_kernel, dim3((unsigned)n_col, gx, (unsigned)zt), dim3(256), 0, c.s, d_batch, d_info, zt, (double)D.mesh.nk, D.n,
                               c.pad, c.nkc, key0, c.d_P, c.d_flag);
            return TBK_OK;
        }
        if (D.n <= 16) return green_launch_invert_np<16>(c, t0, zt, n_col, key0);
        if (D.n <= 32) return green_launch_invert_np<32>(c, t0, zt, n_col, key0);
        return green_launch_invert_np<64>(c, t0, zt, n_col, key0);
    }
};

// The front of both calls on staged handles, behind their checks: the handles opened, per busy handle its slab's k list made and
// uploaded (ws_mesh_k), the slab, and the end of the call.
int green_on_handles(LatticeFamily& fam, tbk_model* const* handles, int n_handles, const int32_t* mesh, int64_t n_r, const int64_t* R, double* G_out) {
    TetraHandles th;
    TBK_CHECK(th.open(handles, n_handles, mesh, OCC_MESH));
    LatticeCall call;  // (in front of the streams)
    MeshStreams streams;
    TBK_CHECK(call.open(fam, th, mesh, n_r, R, G_out, (size_t)th.cut.busy()));
    for (int i = 0; i < th.cut.busy(); ++i) {  // handles whose slab is empty are skipped
        tbk_model* m = handles[i];  // (locked by th)
        std::vector<double>& h_k = call.h_k[(size_t)i];
        TBK_CHECK(streams.add(m));
        TBK_CHECK(tbk_dos_mesh_klist(th.dim, mesh, th.cut.lo(i), th.cut.count(i), &h_k));
        TBK_CHECK(m->ws_mesh_k.reserve(h_k.size() * sizeof(double)));
        TBK_HIP(hipMemcpyAsync(m->ws_mesh_k.ptr, h_k.data(), h_k.size() * sizeof(double), hipMemcpyHostToDevice, m->stream));
        TBK_CHECK(lattice_slab(fam, th, call, (size_t)i, m, &streams.used.back().ev, m->ws_mesh_k.as<double>(), th.cut.count(i) * th.plane_pts,
                               th.cut.lo(i) * th.plane_pts));
    }
    return lattice_finish(fam, call, streams);
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
    DressedFamily fam(n_z, z, Sigma);
    return lattice_from_arrays(fam, dim, mesh, nk, n_orb, nullptr, H, k_chunk, z_tile, n_r, R, G_out);
}

extern "C" int tbk_green_dressed_multi(tbk_model* const* handles, int n_handles, const int32_t* mesh, int64_t n_z, const double* z, const double* Sigma,
                                       int64_t n_r, const int64_t* R, double* G_out) {
    TBK_ARG(handles != nullptr && n_handles >= 1 && handles[0] != nullptr, "no handles");
    TBK_CHECK(green_check_dressed(n_z, z, handles[0]->n_orb, Sigma));
    TBK_CHECK(dm_check_R(n_r, R, G_out, handles[0]->n_orb));
    DressedFamily fam(n_z, z, Sigma);
    return green_on_handles(fam, handles, n_handles, mesh, n_r, R, G_out);
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
    GreenFamily fam(n_z, z);
    return lattice_from_arrays(fam, dim, mesh, nk, n_orb, E, U, k_chunk, z_tile, n_r, R, G_out);
}

extern "C" int tbk_green_function_multi(tbk_model* const* handles, int n_handles, const int32_t* mesh, int64_t n_z, const double* z, int64_t n_r,
                                        const int64_t* R, double* G_out) {
    TBK_CHECK(green_check_z(n_z, z));
    TBK_ARG(handles != nullptr && n_handles >= 1 && handles[0] != nullptr, "no handles");
    TBK_CHECK(dm_check_R(n_r, R, G_out, handles[0]->n_orb));
    GreenFamily fam(n_z, z);
    return green_on_handles(fam, handles, n_handles, mesh, n_r, R, G_out);
}

extern "C" int tbk_green_function(tbk_model* m, const int32_t* mesh, int64_t n_z, const double* z, int64_t n_r, const int64_t* R, double* G_out) {
    return tbk_green_function_multi(&m, 1, mesh, n_z, z, n_r, R, G_out);
}

extern "C" int tbk_green_timing(tbk_model* m, double* ms, int64_t* calls, int reset) {
    TBK_ARG(m != nullptr && ms != nullptr && calls != nullptr, "model / ms / calls is NULL");
    return tbk_timed_read(m, TIMED_GREEN, 3, ms, calls, nullptr, reset);
}
