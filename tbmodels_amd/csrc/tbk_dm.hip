// tbk_dm.hip -- the real-space one-particle density matrix of a uniform, periodic k mesh at one chemical potential.  Not in the
// reference; DESIGN.md section 14 has the quantity, the kernels and the measurements, tools/dm_model.py is the statement the tests
// compare with.
//
//   P(k)[i][j]  = sum_b w[k][b] U[k][i][b] conj(U[k][j][b])              w of tbk_occ.hip at mu, U of tbk_eigh_device (convention 2)
//   rho(R)[i][j] = sum_k exp(-2 pi i  num(k, R) / NK) P(k)[i][j]         num = sum_d ((i_d R_d) mod n_d) (NK / n_d)  mod NK
//
// The phase.  Mesh point k = (i_1 / n_1, ..., i_dim / n_dim).  The host reduces every R_d to [0, n_d) first (so the 64-bit product
// below cannot overflow; (i_d R_d) mod n_d does not change), the kernel forms t_d = (i_d (R_d mod n_d)) mod n_d in 64-bit integers,
// brings the numerators to the common denominator NK = prod n_d < 2^31, num = (sum_d t_d NK / n_d) mod NK, and takes
// sincospi(2 num / NK): one division of two exact integers, nothing else in floating point.  R and R + n_d e_d give the same bits.
//
// Three kernels per chunk of k-points (the eigenvectors come one chunk at a time), all in TABLE coordinates: the chunk holds the
// slab's points [c0, c0 + nkc); table column j is slab point 4 (c0 / 4) + j, so groups of four columns -- one MFMA's K -- start at
// multiples of four of the SLAB index whatever the chunk, up to three leading and three trailing columns are padding (phase 0,
// P 0), and the fixed k slices of the Fourier kernel (multiples of four points) never cut a group.
//
//   dm_phase_kernel    tab[R tile][group][cos | sin][64]: the A operand of the Fourier product in the order its lanes load it --
//                      lane (q, r) of a group holds R row 16 tile + r at column 4 group + q.  VALU work, once per chunk.
//   dm_project_kernel  P = (U diag w) U^H as two real products on v_mfma_f64_16x16x4_f64, contraction over the bands:
//                      Pr = wUr Ur^T + wUi Ui^T, Pi = wUi Ur^T - wUr Ui^T (zmfma_abh of tbk_zmfma.h).  A workgroup
//                      owns a 64 x 64 block of one P(k) (16 x 16 of four k-points up to 16 orbitals): panels of 16 bands of the
//                      block's rows of U go through LDS once, band-major planes wUr, wUi (rows of the block) and Ur, Ui (its
//                      columns), padded with zeros to the tile, so an operand is one ds_read_b64 per lane.  Every tile is computed
//                      (no mirroring).  Padding columns of the table get P = 0.
//   dm_fourier_kernel  rho_r += c Pr + s Pi, rho_i += c Pi - s Pr: one wave per output tile of 16 R-vectors x 16 complex elements of
//                      the n^2, two accumulators, four MFMAs per group of four k-points, operands straight from global memory
//                      (tab: 512 contiguous bytes per load; P: four 256-byte row segments as double2), sixteen MFMAs per pointer bump.
//                      The accumulators start from and return to part[slice][R][n^2], which lives across the chunks of a call:
//                      every element has one owner per launch, no atomics.  Few tiles (8 orbitals: 4 column tiles per 16 R): the
//                      slab's points are cut into `slices` ranges of kps points -- a function of the slab index, not of the chunk,
//                      as in occ_contract_kernel -- one partial rho each, and dm_reduce_kernel adds them in index order.
//
// The plan, the launchers of dm_phase_kernel, dm_fourier_kernel and dm_reduce_kernel and the checks of R are declared in tbk_dm.h:
// the host drivers of tbk_lattice.hip run these three kernels around a family's own projector, this file's or tbk_green.hip's.
//
// For given (w, U), R, chunk size and slab the bits of rho depend on nothing else.  Another chunk size regroups the k-points of the
// groups at the chunk boundaries: results differ within the rounding bound of DESIGN 14.

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "tbk_lattice.h"
#include "tbk_zmfma.h"

namespace {
constexpr int64_t DM_TARGET_WAVES = 1024;  // Fourier tiles x slices the plan aims for (four waves on each of 256 CUs)
constexpr int64_t DM_MIN_SLICE = 16;       // mesh points per slice, at least
}  // namespace

// the slices: enough of them to fill the device with tiles, none shorter than 16 points, all partials inside the budget
static void dm_plan_slices(int64_t rows, int n_orb, int64_t n_r, int64_t* nr_pad, int64_t* slices, int64_t* kps) {
    const int64_t n2 = (int64_t)n_orb * n_orb;
    *nr_pad = (n_r + 15) / 16 * 16;
    const int64_t tiles = *nr_pad / 16 * ((n2 + 15) / 16);
    const int64_t by_work = (DM_TARGET_WAVES + tiles - 1) / tiles;
    const int64_t by_rows = rows / DM_MIN_SLICE;
    const int64_t by_memory = (int64_t)(DM_PART_BUDGET / ((size_t)*nr_pad * n2 * sizeof(double2)));
    const int64_t want = std::max<int64_t>(1, std::min(by_work, std::min(by_rows, by_memory)));
    *kps = ((rows + want - 1) / want + 3) / 4 * 4;
    *slices = std::max<int64_t>(1, (rows + *kps - 1) / *kps);
}

namespace {

__global__ void __launch_bounds__(DM_THREADS) dm_phase_kernel(const int32_t* __restrict__ Rm, DmMesh g, int64_t n_r, int64_t nr_pad, int64_t c0,
                                                              int64_t nkc, int64_t ng, double* __restrict__ tab) {
    const int64_t t = (int64_t)blockIdx.x * DM_THREADS + threadIdx.x;
    if (t >= nr_pad / 16 * ng * 64) return;
    const int lane = (int)(t & 63);
    const int64_t gg = (t >> 6) % ng, rt = (t >> 6) / ng;
    const int64_t r = rt * 16 + (lane & 15);
    const int64_t k = ((c0 >> 2) + gg) * 4 + (lane >> 4);  // in the slab
    double c = 0.0, s = 0.0;
    if (r < n_r && k >= c0 && k < c0 + nkc) {
        int64_t pt = g.first + k, num = 0;
#pragma unroll
        for (int d = 2; d >= 0; --d) {  // (unrolled: the axes are named, the mesh stays in the kernel arguments)
            if (d >= g.dim) continue;
            const int64_t nd = g.n[d];
            const int64_t id = pt % nd;
            pt /= nd;
            const int64_t td = (id * (int64_t)Rm[r * g.dim + d]) % nd;  // both factors in [0, n_d)
            num += td * (g.nk / nd);
        }
        num %= g.nk;
        sincospi((double)(2 * num) / (double)g.nk, &s, &c);
    }
    tab[((rt * ng + gg) * 2 + 0) * 64 + lane] = c;
    tab[((rt * ng + gg) * 2 + 1) * 64 + lane] = s;
}

// BT tiles of 16 along each side of the workgroup's block of P: 4 (one k-point per workgroup, wave t owns tile row t) or 1 (n <= 16:
// four k-points per workgroup, one per wave).  U, w: of the chunk.  Table column j is chunk point j - pad.
template <int BT>
__global__ void __launch_bounds__(DM_THREADS) dm_project_kernel(const double2* __restrict__ U, const double* __restrict__ w, int n, int64_t pad,
                                                                int64_t nkc, double2* __restrict__ P) {
    using Geo = ZPanel<BT>;  // (tbk_zmfma.h; an item is a k-point)
    constexpr int RB = Geo::RB, KPW = Geo::KPW, TEAM = Geo::TEAM, S = Geo::S;
    static_assert(DM_THREADS == Geo::THREADS, "the panel's workgroup");
    __shared__ double planes[KPW][4][16][S];      // wUr, wUi of the block's rows; Ur, Ui of its columns
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int team = BT == 1 ? wave : 0, tt = tid - team * TEAM;
    const int nb = (n + RB - 1) / RB;
    const int bi = (int)blockIdx.y / nb, bj = (int)blockIdx.y - bi * nb;
    const int64_t j = (int64_t)blockIdx.x * KPW + team;  // table column
    const int64_t k = j - pad;
    const bool valid = k >= 0 && k < nkc;
    const double2* Uk = U + (valid ? (size_t)k * n * n : 0);
    const double* wk = w + (valid ? (size_t)k * n : 0);
    double(*pl)[16][S] = planes[team];
    const int ti = BT == 1 ? 0 : wave;  // the wave's tile row
    const bool row_live = bi * RB + ti * 16 < n;  // (wave-uniform)
    zd4 accr[BT], acci[BT];
#pragma unroll
    for (int tj = 0; tj < BT; ++tj) accr[tj] = acci[tj] = zd4{0.0, 0.0, 0.0, 0.0};
    const int sb = tt & 15, srow0 = tt >> 4;
    for (int b0 = 0; b0 < n; b0 += 16) {
        __syncthreads();  // the previous panel has been read
        const int b = b0 + sb;
        const bool b_in = valid && b < n;
        const double wv = b_in ? wk[b] : 0.0;
        for (int row = srow0; row < RB; row += TEAM / 16) {
            const int gi = bi * RB + row, gj = bj * RB + row;
            double2 ui = make_double2(0.0, 0.0), uj = ui;
            if (b_in && gi < n) ui = Uk[(size_t)gi * n + b];
            if (bi == bj)
                uj = ui;
            else if (b_in && gj < n)
                uj = Uk[(size_t)gj * n + b];
            pl[0][sb][row] = wv * ui.x;
            pl[1][sb][row] = wv * ui.y;
            pl[2][sb][row] = uj.x;
            pl[3][sb][row] = uj.y;
        }
        __syncthreads();
        if (row_live) {
#pragma unroll 1
            for (int q = 0; q < 4; ++q) {  // (not unrolled: ZPanel's note on registers)
                const int bq = 4 * q + (lane >> 4);
                const double ar = pl[0][bq][ti * 16 + (lane & 15)], ai = pl[1][bq][ti * 16 + (lane & 15)];
#pragma unroll
                for (int tj = 0; tj < BT; ++tj) {
                    if (bj * RB + tj * 16 < n) {  // (uniform)
                        const double br = pl[2][bq][tj * 16 + (lane & 15)], bim = pl[3][bq][tj * 16 + (lane & 15)];
                        zmfma_abh(ar, ai, br, bim, accr[tj], acci[tj]);
                    }
                }
            }
        }
    }
    if (!row_live) return;
    ztiles_store<BT>(P + (size_t)j * n * n, n, bi * RB + ti * 16, bj * RB, lane, accr, acci);
}

__device__ __forceinline__ void dm_fourier_step(double c, double s, double2 p, zd4& ar, zd4& ai) {
    zmfma_ahb(c, s, p.x, p.y, ar, ai);  // (c + i s)^H (Pr + i Pi)
}

// grid: (column tiles / 4, R tiles, slices the chunk touches from slice_lo on); a wave owns one tile of one slice.  The chunk's table
// holds the absolute groups [g0, g_end) of the slab, slice s owns [s gps, (s + 1) gps).
__global__ void __launch_bounds__(DM_THREADS) dm_fourier_kernel(const double* __restrict__ tab, const double2* __restrict__ P, int64_t n2, int64_t nct,
                                                                int64_t nr_pad, int64_t ng, int64_t g0, int64_t g_end, int64_t gps,
                                                                int64_t slice_lo, double2* __restrict__ part) {
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int64_t ct = (int64_t)blockIdx.x * 4 + wave;
    if (ct >= nct) return;
    const int64_t rt = blockIdx.y, sl = slice_lo + blockIdx.z;
    const int64_t ga = max(g0, sl * gps), gb = min(g_end, (sl + 1) * gps);
    if (ga >= gb) return;
    const int64_t e = ct * 16 + (lane & 15);  // the lane's element of the n^2, as B column and as column of the result
    const bool e_in = e < n2;
    const double* pa = tab + ((rt * ng + (ga - g0)) * 2) * 64 + lane;
    const double2* pb = P + ((ga - g0) * 4 + (lane >> 4)) * n2 + (e_in ? e : n2 - 1);
    double2* out = part + ((sl * nr_pad + rt * 16 + (lane >> 4)) * n2 + e);  // register r: 4 r rows further
    const int64_t out_step = 4 * n2, p_step = 4 * n2;
    zd4 ar = {0.0, 0.0, 0.0, 0.0}, ai = ar;
    if (e_in) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double2 z = out[r * out_step];
            ar[r] = z.x;
            ai[r] = z.y;
        }
    }
    int64_t cnt = gb - ga;
    for (; cnt >= 4; cnt -= 4) {
        double c[4], s[4];
        double2 p[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            c[u] = pa[u * 128];
            s[u] = pa[u * 128 + 64];
            p[u] = pb[u * p_step];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) dm_fourier_step(c[u], s[u], p[u], ar, ai);
        pa += 4 * 128;
        pb += 4 * p_step;
    }
    for (; cnt > 0; --cnt) {
        dm_fourier_step(pa[0], pa[64], pb[0], ar, ai);
        pa += 128;
        pb += p_step;
    }
    if (e_in) {
#pragma unroll
        for (int r = 0; r < 4; ++r) out[r * out_step] = make_double2(ar[r], ai[r]);
    }
}

// rho[r][e] = the slices' partials in index order
__global__ void __launch_bounds__(DM_THREADS) dm_reduce_kernel(const double2* __restrict__ part, int64_t slices, int64_t nr_pad, int64_t n_r, int64_t n2,
                                                               double2* __restrict__ rho) {
    const int64_t idx = (int64_t)blockIdx.x * DM_THREADS + threadIdx.x;
    if (idx >= n_r * n2) return;
    double2 acc = part[idx];  // (rows of slice 0 are those of rho)
    for (int64_t s = 1; s < slices; ++s) {
        const double2 z = part[s * nr_pad * n2 + idx];
        acc.x += z.x;
        acc.y += z.y;
    }
    rho[idx] = acc;
}

}  // namespace

// ---- host ----------------------------------------------------------------------------------------------------------------------
int dm_plan(int dim, const int32_t* mesh, int64_t nk_total, int64_t first_pt, int64_t rows, int n_orb, int64_t n_r, DmPlan* out) {
    DmPlan L;
    L.mesh.dim = dim;
    L.mesh.n[0] = mesh[0];
    L.mesh.n[1] = mesh[1];
    L.mesh.n[2] = dim == 3 ? mesh[2] : 1;
    L.mesh.nk = nk_total;
    L.mesh.first = first_pt;
    L.n = n_orb;
    L.n2 = (int64_t)n_orb * n_orb;
    L.nct = (L.n2 + 15) / 16;
    L.n_r = n_r;
    L.rows = rows;
    dm_plan_slices(rows, n_orb, n_r, &L.nr_pad, &L.slices, &L.kps);
    *out = L;
    return TBK_OK;
}

// R[n_r][dim] reduced to [0, n_d) per axis
int dm_reduce_R(int dim, const int32_t* mesh, int64_t n_r, const int64_t* R, std::vector<int32_t>* out) {
    try {
        out->resize((size_t)n_r * dim);
    } catch (...) {
        tbk_set_error("cannot allocate the reduced lattice vectors");
        return TBK_ERR_MEMORY;
    }
    for (int64_t r = 0; r < n_r; ++r)
        for (int d = 0; d < dim; ++d) {
            const int64_t nd = mesh[d];
            (*out)[(size_t)r * dim + d] = (int32_t)(((R[r * dim + d] % nd) + nd) % nd);
        }
    return TBK_OK;
}

// a chunk no longer than the phase table's budget allows
int64_t dm_cap_chunk(const DmPlan& L, int64_t chunk) {
    const int64_t by_tab = (int64_t)(DM_TAB_BUDGET / ((size_t)L.nr_pad * 2 * sizeof(double)));
    return std::max<int64_t>(1, std::min(chunk, std::max<int64_t>(4, by_tab - 8)));
}

int dm_launch_phase(hipStream_t s, const DmPlan& L, SpanRecorder* ev, const int32_t* d_Rm, int64_t c0, int64_t nkc, double* d_tab) {
    const int64_t pad = c0 & 3, ng = (pad + nkc + 3) / 4;
    const int64_t tab_threads = L.nr_pad / 16 * ng * 64;
    if (ev) ev->start(0);
    hipLaunchKernelGGL(dm_phase_kernel, dim3((unsigned)((tab_threads + DM_THREADS - 1) / DM_THREADS)), dim3(DM_THREADS), 0, s, d_Rm, L.mesh, L.n_r,
                       L.nr_pad, c0, nkc, ng, d_tab);
    if (ev) ev->stop();
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

int dm_launch_fourier(hipStream_t s, const DmPlan& L, SpanRecorder* ev, int64_t c0, int64_t nkc, const double* d_tab, const double2* d_P,
                      double2* d_part) {
    const int64_t pad = c0 & 3, g0 = c0 >> 2, ng = (pad + nkc + 3) / 4, g_end = g0 + ng, gps = L.kps / 4;
    const int64_t slice_lo = g0 / gps, slice_hi = (g_end - 1) / gps;
    if (ev) ev->start(2);
    hipLaunchKernelGGL(dm_fourier_kernel, dim3((unsigned)((L.nct + 3) / 4), (unsigned)(L.nr_pad / 16), (unsigned)(slice_hi - slice_lo + 1)),
                       dim3(DM_THREADS), 0, s, d_tab, d_P, L.n2, L.nct, L.nr_pad, ng, g0, g_end, gps, slice_lo, d_part);
    if (ev) ev->stop();
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

// the result of the slab in device memory: d_part itself with one slice, else the slices summed into d_rho
int dm_launch_reduce(hipStream_t s, const DmPlan& L, SpanRecorder* ev, const double2* d_part, double2* d_rho, const double2** result) {
    *result = d_part;
    if (L.slices == 1) return TBK_OK;
    if (ev) ev->start(2);
    hipLaunchKernelGGL(dm_reduce_kernel, dim3((unsigned)((L.n_r * L.n2 + DM_THREADS - 1) / DM_THREADS)), dim3(DM_THREADS), 0, s, d_part, L.slices,
                       L.nr_pad, L.n_r, L.n2, d_rho);
    if (ev) ev->stop();
    TBK_HIP(hipGetLastError());
    *result = d_rho;
    return TBK_OK;
}

int dm_check_R(int64_t n_r, const int64_t* R, const double* rho_out, int n_orb) {
    TBK_ARG(n_r >= 1, "n_r < 1");
    TBK_ARG(R != nullptr && rho_out != nullptr, "R / rho is NULL");
    TBK_ARG(n_r <= DM_MAX_R, "more than 1048560 lattice vectors in one call");
    TBK_ARG(n_orb <= 16320, "more than 16320 orbitals");  // (255 x 255 blocks of the projector: one grid row each)
    return TBK_OK;
}

extern "C" int tbk_dm_plan(int64_t rows, int n_orb, int64_t n_r, int64_t* out) {
    TBK_ARG(rows >= 1 && n_orb >= 1 && n_r >= 1 && out != nullptr, "rows / n_orb / n_r < 1 or out is NULL");
    dm_plan_slices(rows, n_orb, n_r, &out[0], &out[1], &out[2]);
    return TBK_OK;
}

namespace {

// The density matrix as the drivers of tbk_lattice.h see it: one energy in one tile, P = U diag(w) U^H from the chunk's eigenvectors
// and its rows of the point weights w, which the entry point makes for the whole slab first.
struct DmFamily : LatticeFamily {
    const double* d_w = nullptr;  // the slab's weights [rows][n]
    DmFamily() : LatticeFamily(TIMED_DM) {}
    // no budget for P beside the phase table's: the chunk is the option, else the automatic one
    GreenPlan plan(const DmPlan& D, int64_t, int64_t k_chunk, int64_t auto_chunk) const override {
        GreenPlan G;
        G.D = D;
        G.bt = D.n <= 16 ? 1 : 4;
        G.gather = false;
        G.chunk = dm_cap_chunk(D, k_chunk > 0 ? std::min(k_chunk, D.rows) : auto_chunk);
        return G;
    }
    int share(int, bool) const override { return 2; }  // the chunk is halved for the P buffer
    int fill_p(const LatticeChunk& c, int64_t) const override {
        const int n = c.G.D.n;
        const double2* U = reinterpret_cast<const double2*>(c.d_in);
        const double* w = d_w + (size_t)c.c0 * n;
        if (c.G.bt == 1)
            hipLaunchKernelGGL(dm_project_kernel<1>, c.project_grid(), dim3(DM_THREADS), 0, c.s, U, w, n, c.pad, c.nkc, c.d_P);
        else
            hipLaunchKernelGGL(dm_project_kernel<4>, c.project_grid(), dim3(DM_THREADS), 0, c.s, U, w, n, c.pad, c.nkc, c.d_P);
        return TBK_OK;
    }
};

}  // namespace

extern "C" int tbk_density_matrix_from_eigensystem(int device, int dim, const int32_t* mesh, int n_orb, const double* E, const double* U,
                                                   double energy, int64_t k_chunk, int64_t n_r, const int64_t* R, double* rho_out) {
    int64_t nk = 0;
    TBK_CHECK(tetra_check_mesh(dim, mesh, OCC_MESH, &nk));
    TBK_ARG(E != nullptr && U != nullptr, "E / U is NULL");
    TBK_ARG(n_orb >= 1, "n_orb < 1");
    TBK_ARG(std::isfinite(energy), "the energy is not finite");
    TBK_ARG(k_chunk >= 0, "k_chunk < 0");
    TBK_CHECK(dm_check_R(n_r, R, rho_out, n_orb));
    TBK_CHECK(tetra_check_device(device));
    // the weights of the whole mesh from its eigenvalues, once; the driver walks the eigenvectors
    OccPlan L;
    TBK_CHECK(occ_plan(dim, mesh, mesh[0], mesh[0], 0, n_orb, &L));
    const size_t e_bytes = (size_t)nk * (size_t)n_orb * sizeof(double);
    DevBuf d_E, d_w;
    TBK_CHECK(d_E.reserve(e_bytes));
    TBK_CHECK(d_w.reserve(e_bytes));
    TBK_HIP(hipMemcpy(d_E.ptr, E, e_bytes, hipMemcpyHostToDevice));
    TBK_CHECK(occ_launch_weights(nullptr, L, d_E.as<double>(), energy, (double)nk, d_w.as<double>()));
    DmFamily fam;
    fam.d_w = d_w.as<double>();
    return lattice_from_arrays(fam, dim, mesh, nk, n_orb, nullptr, U, k_chunk, 0, n_r, R, rho_out);
}

extern "C" int tbk_density_matrix_multi(tbk_model* const* handles, int n_handles, const int32_t* mesh, int mode, double value, int64_t n_r,
                                        const int64_t* R, double* mu_out, double* rho_out) {
    TBK_ARG(mu_out != nullptr, "mu is NULL");
    TBK_ARG(mode == 0 || mode == 1, "mode must be 0 (value = energy) or 1 (value = n_electrons)");
    TBK_ARG(handles != nullptr && n_handles >= 1 && handles[0] != nullptr, "no handles");
    TBK_CHECK(dm_check_R(n_r, R, rho_out, handles[0]->n_orb));
    if (mode == 1)
        TBK_CHECK(tbk_fermi_check_electrons(value, handles[0]->n_orb));
    else
        TBK_ARG(std::isfinite(value), "the energy is not finite");
    DmFamily fam;
    LatticeCall call;  // (in front of the staged call, which holds the streams)
    OccStaged staged;
    TBK_CHECK(staged.make(handles, n_handles, mesh));
    TBK_CHECK(staged.find_mu(mesh, mode, value, mu_out));
    TBK_CHECK(staged.weights(mu_out[0], nullptr, false));  // (not one of this family's three stages: not timed)
    TBK_CHECK(call.open(fam, staged, mesh, n_r, R, rho_out, staged.slabs.size()));
    for (size_t i = 0; i < staged.slabs.size(); ++i) {
        TetraSlab& s = staged.slabs[i];
        TBK_HIP(hipSetDevice(s.m->device));
        fam.d_w = s.m->ws_occ_w.as<double>();
        // (the slab's own k list is the eigenvalue path's, behind the neighbour plane)
        const double* d_k_own = s.m->ws_k.as<double>() + (size_t)s.head * staged.dim;
        TBK_CHECK(lattice_slab(fam, staged, call, i, s.m, s.ev, d_k_own, staged.occ[i].L.rows, s.p_lo * staged.plane_pts));
    }
    return lattice_finish(fam, call, staged.streams);
}

extern "C" int tbk_density_matrix(tbk_model* m, const int32_t* mesh, int mode, double value, int64_t n_r, const int64_t* R, double* mu_out,
                                  double* rho_out) {
    return tbk_density_matrix_multi(&m, 1, mesh, mode, value, n_r, R, mu_out, rho_out);
}

extern "C" int tbk_dm_timing(tbk_model* m, double* ms, int64_t* calls, int reset) {
    TBK_ARG(m != nullptr && ms != nullptr && calls != nullptr, "model / ms / calls is NULL");
    return tbk_timed_read(m, TIMED_DM, 3, ms, calls, nullptr, reset);
}
