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

#include <algorithm>
#include <cmath>
#include <vector>

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

}  // namespace

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
