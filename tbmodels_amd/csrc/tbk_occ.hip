// tbk_occ.hip -- the tetrahedron integration weight of every state (k, b) of a uniform, periodic k mesh at one energy mu, and what a
// user integrates with it: band occupations, band energies and the charge on every orbital.  Not in the reference; DESIGN.md
// section 13 has the quantities, the summation orders and the measurements, tools/occ_model.py is the statement the tests compare with.
// (The plan of a slab, the launchers below and the staged call -- handles, slabs, eigenvalues, mu, weights -- are declared in tbk_occ.h:
// tbk_dm.hip drives the same call up to the weights.)
//
//   E[planes][n1][n2][n_orb]  ascending eigenvalues per mesh point, mesh order (last axis fastest): what tbk_dos.hip reads
//   w[k][b]   = (sum over the simplices T that contain mesh point k of Bloechl's corner weight w_c(T, b; mu) of k in T) / (S NK)
//   f[b]      = sum_k w[k][b]                       eb[b] = sum_k w[k][b] E[k][b]
//   q[i]      = sum_k sum_b w[k][b] |U[k][i][b]|^2  (U[nk][n][n][2] of tbk_eigh_device, convention 2)
//
// tetra_weights_kernel is a GATHER: the work item is one (mesh point, band) pair, band fastest, so a wave reads 64 consecutive
// doubles of a row of E per neighbour.  Mesh point v is corner p of the simplex with axis order sigma of the cell at
// v - (e_sigma1 + ... + e_sigmap): in three dimensions 6 orders x 4 positions = 24 tetrahedra over v and the 14 offsets in
// {-1, 0, 1}^3 whose non-zero components share a sign, in two dimensions 2 x 3 = 6 triangles over 7 points.  The item loads those 15
// (7) energies once, walks the simplices in the order s = 4 sigma + p (3 sigma + p), sigma in the order of tbk_dos.hip's list
// (012, 021, 102, 120, 201, 210; 01, 10), by two nested loops that are NOT unrolled -- the corners are selected by uniform indices, so
// the branch code exists once -- and adds the own corner's weight of every simplex to ONE double in that order.  Per simplex: the
// stable sort of tbk_tetra.h (adjacent exchanges on a strict comparison, corners in simplex order) carrying the rank of the own
// corner; 0 or the full weight from two comparisons unless e1 <= mu < e_top; else the reciprocals of the DOS_GAP_SCALE-scaled gaps
// and the corner weights that pdos_simplex takes as well: TetraGaps::corner_weights.  A full tetrahedron gives 1/4 to every corner, so above the
// spectrum the sum is 24 / 4 = 6 exactly and w = 6 / (6 NK) is the double nearest 1 / NK.  A triangle's corner weights are carried
// TIMES THREE (a full corner is 1, not the inexact 1/3) and the divisor is 3 S NK = 6 NK: the same property.  One division, one
// plain store per item: no atomics, no LDS, no scratch; for given E and mu the bits of w depend on nothing else.
//
// Every axis goes through the same modular neighbour index (i - 1 and i + 1 modulo the planes held): an axis of one point is its
// own neighbour on both sides, an axis of two has one neighbour on both sides.  A slab of a mesh shared among handles holds the
// periodic neighbour plane on BOTH sides of its own planes (off0 = 1): the modular index then never wraps along axis 0.
//
// occ_band_kernel: f in the 64-bit fixed point of DESIGN 10.3 -- a term is round(NK w 2^40) -- and eb in doubles in a fixed order:
// the own mesh points are cut into blocks of 256 consecutive points; inside a block the lane of band b with row slot r (of
// 256 / n_orb slots; one above 256 orbitals) adds the points r, r + slots, ... in index order, the slots are added in index order,
// and occ_band_reduce_kernel adds the blocks in index order.  So eb depends on (slab, n_orb) alone and f on nothing but w.
//
// occ_contract_kernel: one wave per (k, i) row of U, lanes along b (16-byte loads, coalesced; w[k][.] alongside).  A lane adds its
// bands b = lane, lane + 64, ... in order, the lanes meet in an xor butterfly (32, 16, ..., 1: commutative, every lane holds the same
// bits), P = NK * sum in [0, 1] is rounded ONCE to fixed point and added, in integers, to the workgroup's LDS accumulator of orbital
// i; the workgroup then adds its accumulators to its own row of a [n_workgroups][n_orb] buffer that persists across the k chunks of a
// call.  Which workgroup takes a k-point is a function of the point's index in the slab (kpw consecutive points each, at most 2^20:
// a row's sums stay below 2^60), not of the chunk.  occ_reduce_kernel sums the rows, high 44 and low 20 bits apart.  For given
// (w, U) the bits of q depend neither on the chunk size nor on the workgroup count; |error| <= 2^-41 per orbital.

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "tbk_occ.h"

namespace {

constexpr int OCC_THREADS = 256;
constexpr int OCC_BLOCK = 256;             // mesh points per block of the band sums
constexpr int64_t OCC_MAX_WG = 4096;       // rows of the contraction buffer, at most (more only for the 2^20 bound)
constexpr int64_t OCC_MAX_GRID = 1 << 20;  // workgroups of the weights kernel, at most (the items are strided over them)

__device__ __forceinline__ int occ_prev(int i, int n) { return i == 0 ? n - 1 : i - 1; }
__device__ __forceinline__ int occ_next(int i, int n) { return i + 1 == n ? 0 : i + 1; }

// the payload of the stable sort (tbk_tetra.h): the rank of the own corner
struct OccRank {
    int r;
    template <int A, int B>
    __device__ __forceinline__ void follow(bool sw) {
        r = sw ? (r == A ? B : r == B ? A : r) : r;
    }
};

// Bloechl's weight of corner `own` (0 .. NC - 1, in simplex order) of one simplex at mu.  A tetrahedron's is in [0, 1/4]; a
// triangle's is carried TIMES THREE: in [0, 1], exactly 1 for a full triangle.
template <int NC>
__device__ __forceinline__ double occ_simplex(const double (&corners)[NC], int own, double mu) {
    constexpr double full = NC == 4 ? 0.25 : 1.0;
    double e[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) e[c] = corners[c];
    OccRank rank{own};
    tetra_stable_sort(e, rank);
    if (mu < e[0]) return 0.0;
    if (mu >= e[NC - 1]) return full;
    const TetraGaps<NC> gaps(e);
    double wc[NC];
    if constexpr (NC == 4)
        gaps.corner_weights(mu, wc);
    else
        gaps.template corner_weights<1>(mu, wc);
    const int r = rank.r;
    const double w = r == 0 ? wc[0] : r == 1 ? wc[1] : NC == 3 || r == 2 ? wc[2] : wc[NC - 1];
    return fmin(fmax(w, 0.0), full);  // (NaN -> 0)
}

__device__ __forceinline__ double occ_pick(int i, double x, double y, double z) { return i == 0 ? x : i == 1 ? y : z; }

// w[own point][n_orb] = acc / denom, denom = 24 NK / 4 = 6 NK in both dimensions (see the head of the file)
template <int DIM>
__global__ void __launch_bounds__(OCC_THREADS) tetra_weights_kernel(const double* __restrict__ E, OccGeom g, double mu, double denom,
                                                                    double* __restrict__ w) {
    for (int64_t it = (int64_t)blockIdx.x * OCC_THREADS + threadIdx.x; it < g.items; it += (int64_t)gridDim.x * OCC_THREADS) {
        const int64_t pt = it / g.n_orb;
        const int band = (int)(it - pt * g.n_orb);
        int c = (int)pt;  // NK < 2^31 (checked by the launcher)
        const int i2 = c % g.n2;
        c /= g.n2;
        const int i1 = c % g.n1;
        const int i0 = c / g.n1 + g.off0;
        const int m0 = occ_prev(i0, g.n0_planes), p0 = occ_next(i0, g.n0_planes);
        const int m1 = occ_prev(i1, g.n1), p1 = occ_next(i1, g.n1);
        auto at = [&](int a0, int a1, int a2) -> double {
            const int64_t k = ((int64_t)a0 * g.n1 + a1) * g.n2 + a2;
            return E[k * g.n_orb + band];
        };
        double acc = 0.0;
        if (DIM == 3) {
            const int m2 = occ_prev(i2, g.n2), p2 = occ_next(i2, g.n2);
            // v, and the neighbours at +x, +y, +z, +x+y, ... (x, y, z = a step along axis 0, 1, 2) and at the negated offsets
            const double v = at(i0, i1, i2);
            const double px = at(p0, i1, i2), py = at(i0, p1, i2), pz = at(i0, i1, p2);
            const double pxy = at(p0, p1, i2), pxz = at(p0, i1, p2), pyz = at(i0, p1, p2), pxyz = at(p0, p1, p2);
            const double mx = at(m0, i1, i2), my = at(i0, m1, i2), mz = at(i0, i1, m2);
            const double mxy = at(m0, m1, i2), mxz = at(m0, i1, m2), myz = at(i0, m1, m2), mxyz = at(m0, m1, m2);
#pragma unroll 1
            for (int o = 0; o < 6; ++o) {
                // the order (a, b, c) of the axes: 012, 021, 102, 120, 201, 210
                const int a = o >> 1;
                const int b = o == 0 || o == 5 ? 1 : o == 1 || o == 3 ? 2 : 0;
                const int cc = 3 - a - b;
                const double pa = occ_pick(a, px, py, pz), pb = occ_pick(b, px, py, pz), pc = occ_pick(cc, px, py, pz);
                const double pab = occ_pick(cc, pyz, pxz, pxy), pbc = occ_pick(a, pyz, pxz, pxy);  // a pair is the complement of an axis
                const double ma = occ_pick(a, mx, my, mz), mb = occ_pick(b, mx, my, mz), mc = occ_pick(cc, mx, my, mz);
                const double mab = occ_pick(cc, myz, mxz, mxy), mbc = occ_pick(a, myz, mxz, mxy);
#pragma unroll 1
                for (int p = 0; p < 4; ++p) {
                    // the cell at v - (e_a + ... ): corners 0, e_a, e_a + e_b, e_a + e_b + e_c of it; v is corner p
                    const double c0 = p == 0 ? v : p == 1 ? ma : p == 2 ? mab : mxyz;
                    const double c1 = p == 0 ? pa : p == 1 ? v : p == 2 ? mb : mbc;
                    const double c2 = p == 0 ? pab : p == 1 ? pb : p == 2 ? v : mc;
                    const double c3 = p == 0 ? pxyz : p == 1 ? pbc : p == 2 ? pc : v;
                    acc += occ_simplex<4>({c0, c1, c2, c3}, p, mu);
                }
            }
        } else {
            const double v = at(i0, i1, 0);
            const double px = at(p0, i1, 0), py = at(i0, p1, 0), pxy = at(p0, p1, 0);
            const double mx = at(m0, i1, 0), my = at(i0, m1, 0), mxy = at(m0, m1, 0);
#pragma unroll 1
            for (int o = 0; o < 2; ++o) {
                const double pa = o == 0 ? px : py, pb = o == 0 ? py : px;
                const double ma = o == 0 ? mx : my, mb = o == 0 ? my : mx;
#pragma unroll 1
                for (int p = 0; p < 3; ++p) {
                    const double c0 = p == 0 ? v : p == 1 ? ma : mxy;
                    const double c1 = p == 0 ? pa : p == 1 ? v : mb;
                    const double c2 = p == 0 ? pxy : p == 1 ? pb : v;
                    acc += occ_simplex<3>({c0, c1, c2}, p, mu);
                }
            }
        }
        w[it] = acc / denom;
    }
}

// grid: (blocks of OCC_BLOCK own mesh points, blocks of 256 bands above 256 orbitals).  part_f / part_eb: [gridDim.x][n_orb]
__global__ void __launch_bounds__(OCC_THREADS) occ_band_kernel(const double* __restrict__ w, const double* __restrict__ E, int64_t rows, int n_orb,
                                                               double nk_total, unsigned long long* __restrict__ part_f,
                                                               double* __restrict__ part_eb) {
    __shared__ double s_eb[OCC_THREADS];
    __shared__ unsigned long long s_f[OCC_THREADS];
    const int tid = (int)threadIdx.x;
    const int slots = n_orb <= OCC_THREADS ? OCC_THREADS / n_orb : 1;
    const int width = n_orb <= OCC_THREADS ? n_orb : min(OCC_THREADS, n_orb - (int)blockIdx.y * OCC_THREADS);
    const int slot = tid / width, lane_band = tid - slot * width;
    const int band = (int)blockIdx.y * OCC_THREADS + lane_band;
    const int64_t r0 = (int64_t)blockIdx.x * OCC_BLOCK, r1 = min(r0 + OCC_BLOCK, rows);
    double eb = 0.0;
    unsigned long long f = 0ull;
    if (slot < slots) {
        for (int64_t r = r0 + slot; r < r1; r += slots) {
            const double x = w[r * n_orb + band];
            eb += x * E[r * n_orb + band];
            f += dos_fixed(x * nk_total);
        }
    }
    s_eb[tid] = eb;
    s_f[tid] = f;
    __syncthreads();
    if (tid < width) {
        for (int q = 1; q < slots; ++q) {
            eb += s_eb[q * width + tid];
            f += s_f[q * width + tid];
        }
        part_eb[(int64_t)blockIdx.x * n_orb + band] = eb;
        part_f[(int64_t)blockIdx.x * n_orb + band] = f;
    }
}

// one thread per band over the blocks in index order.  sums: f high [n_orb], f low [n_orb]; eb [n_orb]
__global__ void __launch_bounds__(OCC_THREADS) occ_band_reduce_kernel(const unsigned long long* __restrict__ part_f, const double* __restrict__ part_eb,
                                                                      int64_t n_blocks, int n_orb, unsigned long long* __restrict__ sums,
                                                                      double* __restrict__ eb_out) {
    const int band = (int)blockIdx.x * OCC_THREADS + (int)threadIdx.x;
    if (band >= n_orb) return;
    DosWords f;
    double eb = 0.0;
    for (int64_t blk = 0; blk < n_blocks; ++blk) {
        f.add(part_f[blk * n_orb + band]);
        eb += part_eb[blk * n_orb + band];
    }
    sums[band] = f.hi;
    sums[n_orb + band] = f.lo;
    eb_out[band] = eb;
}

// U: the eigenvectors of the k-points [c0, c0 + nkc) of the slab's own points, w_chunk their rows of w.  Workgroup blockIdx.x + wg_lo
// owns the points [wg kpw, (wg + 1) kpw) of the slab and takes those of them the chunk holds.  Dynamic LDS: n u64
__global__ void __launch_bounds__(OCC_THREADS) occ_contract_kernel(const double2* __restrict__ U, const double* __restrict__ w_chunk, int n,
                                                                   int64_t c0, int64_t nkc, int64_t kpw, int64_t wg_lo, double nk_total,
                                                                   unsigned long long* __restrict__ buf) {
    extern __shared__ unsigned long long occ_acc[];
    const int tid = (int)threadIdx.x;
    const int64_t wg = wg_lo + blockIdx.x;
    const int64_t k_lo = max(c0, wg * kpw), k_hi = min(c0 + nkc, (wg + 1) * kpw);
    if (k_lo >= k_hi) return;  // (uniform)
    for (int i = tid; i < n; i += OCC_THREADS) occ_acc[i] = 0ull;
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    const int64_t n_rows = (k_hi - k_lo) * n;
    for (int64_t row = wave; row < n_rows; row += OCC_THREADS / 64) {
        const int64_t kk = row / n;
        const int i = (int)(row - kk * n);
        const int64_t k = k_lo - c0 + kk;  // inside the chunk
        const double2* u = U + ((size_t)k * n + i) * n;
        const double* wk = w_chunk + (size_t)k * n;
        double s = 0.0;
        for (int b = lane; b < n; b += 64) {
            const double2 z = u[b];
            const double a = z.x * z.x + z.y * z.y;
            s += wk[b] * a;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
        if (lane == 0) atomicAdd(&occ_acc[i], dos_fixed(s * nk_total));
    }
    __syncthreads();
    for (int i = tid; i < n; i += OCC_THREADS) buf[wg * n + i] += occ_acc[i];  // this workgroup's own row
}

// one thread per orbital over the workgroups' rows.  sums: high [n], low [n]
__global__ void __launch_bounds__(OCC_THREADS) occ_reduce_kernel(const unsigned long long* __restrict__ buf, int64_t n_wg, int n,
                                                                 unsigned long long* __restrict__ sums) {
    const int i = (int)blockIdx.x * OCC_THREADS + (int)threadIdx.x;
    if (i >= n) return;
    DosWords q;
    for (int64_t wg = 0; wg < n_wg; ++wg) q.add(buf[wg * n + i]);
    sums[i] = q.hi;
    sums[n + i] = q.lo;
}

}  // namespace

// ---- host: one slab of the mesh on one device (declared in tbk_occ.h) -----------------------------------------------------------
// cells0 own planes along axis 0 out of planes0 planes in E, the first own one at off0
int occ_plan(int dim, const int32_t* mesh, int64_t cells0, int64_t planes0, int off0, int n_orb, OccPlan* out) {
    OccPlan L;
    L.dim = dim;
    L.g.n0_own = (int)cells0;
    L.g.n0_planes = (int)planes0;
    L.g.off0 = off0;
    L.g.n1 = mesh[1];
    L.g.n2 = dim == 3 ? mesh[2] : 1;
    L.g.n_orb = n_orb;
    L.rows = cells0 * L.g.n1 * L.g.n2;
    L.g.items = L.rows * n_orb;
    L.w_grid = (int)std::min<int64_t>((L.g.items + OCC_THREADS - 1) / OCC_THREADS, OCC_MAX_GRID);
    L.n_blocks = (L.rows + OCC_BLOCK - 1) / OCC_BLOCK;
    // rows of the contraction buffer: at most 32 MiB of them, never more than 2^20 k-points each
    int64_t n_wg = std::min<int64_t>(L.rows, std::min<int64_t>(OCC_MAX_WG, std::max<int64_t>(1, (int64_t(1) << 22) / n_orb)));
    n_wg = std::max<int64_t>(n_wg, (L.rows + DOS_MAX_ITEMS - 1) / DOS_MAX_ITEMS);
    L.kpw = (L.rows + n_wg - 1) / n_wg;
    L.n_wg = (L.rows + L.kpw - 1) / L.kpw;
    const size_t n = (size_t)n_orb;
    L.off_part_eb = dos_align256((size_t)L.n_blocks * n * sizeof(unsigned long long));
    L.off_buf = L.off_part_eb + dos_align256((size_t)L.n_blocks * n * sizeof(double));
    L.off_host = L.off_buf + dos_align256((size_t)L.n_wg * n * sizeof(unsigned long long));
    L.host_bytes = 5 * n * sizeof(double);
    L.ws_bytes = L.off_host + dos_align256(L.host_bytes);
    *out = L;
    return TBK_OK;
}

int occ_launch_weights(hipStream_t s, const OccPlan& L, const double* d_E, double mu, double nk_total, double* d_w) {
    const double denom = 6.0 * nk_total;
    if (L.dim == 3)
        hipLaunchKernelGGL(tetra_weights_kernel<3>, dim3((unsigned)L.w_grid), dim3(OCC_THREADS), 0, s, d_E, L.g, mu, denom, d_w);
    else
        hipLaunchKernelGGL(tetra_weights_kernel<2>, dim3((unsigned)L.w_grid), dim3(OCC_THREADS), 0, s, d_E, L.g, mu, denom, d_w);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

// d_E_own: the rows of E of the own mesh points
int occ_launch_band(hipStream_t s, const OccPlan& L, const double* d_w, const double* d_E_own, double nk_total, char* ws) {
    const int n = L.g.n_orb;
    auto* part_f = reinterpret_cast<unsigned long long*>(ws);
    auto* part_eb = reinterpret_cast<double*>(ws + L.off_part_eb);
    auto* sums = reinterpret_cast<unsigned long long*>(ws + L.off_host);
    auto* eb = reinterpret_cast<double*>(ws + L.off_host) + 4 * (size_t)n;
    const dim3 grid((unsigned)L.n_blocks, (unsigned)((n + OCC_THREADS - 1) / OCC_THREADS));
    hipLaunchKernelGGL(occ_band_kernel, grid, dim3(OCC_THREADS), 0, s, d_w, d_E_own, L.rows, n, nk_total, part_f, part_eb);
    TBK_HIP(hipGetLastError());
    hipLaunchKernelGGL(occ_band_reduce_kernel, dim3(grid.y), dim3(OCC_THREADS), 0, s, part_f, part_eb, L.n_blocks, n, sums, eb);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

int occ_clear_buf(hipStream_t s, const OccPlan& L, char* ws) {
    TBK_HIP(hipMemsetAsync(ws + L.off_buf, 0, (size_t)L.n_wg * (size_t)L.g.n_orb * sizeof(unsigned long long), s));
    return TBK_OK;
}

// the own points [c0, c0 + nkc) of the slab: d_U their eigenvectors, d_w the slab's weights
int occ_launch_contract(hipStream_t s, const OccPlan& L, const double* d_U, const double* d_w, int64_t c0, int64_t nkc, double nk_total, char* ws) {
    const int n = L.g.n_orb;
    const int64_t wg_lo = c0 / L.kpw, wg_hi = (c0 + nkc - 1) / L.kpw;
    hipLaunchKernelGGL(occ_contract_kernel, dim3((unsigned)(wg_hi - wg_lo + 1)), dim3(OCC_THREADS), (size_t)n * sizeof(unsigned long long), s,
                       reinterpret_cast<const double2*>(d_U), d_w + (size_t)c0 * n, n, c0, nkc, L.kpw, wg_lo, nk_total,
                       reinterpret_cast<unsigned long long*>(ws + L.off_buf));
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

int occ_launch_reduce(hipStream_t s, const OccPlan& L, char* ws) {
    const int n = L.g.n_orb;
    hipLaunchKernelGGL(occ_reduce_kernel, dim3((unsigned)((n + OCC_THREADS - 1) / OCC_THREADS)), dim3(OCC_THREADS), 0, s,
                       reinterpret_cast<const unsigned long long*>(ws + L.off_buf), L.n_wg, n,
                       reinterpret_cast<unsigned long long*>(ws + L.off_host) + 2 * (size_t)n);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

namespace {

// the integer words of f and q and the doubles of eb, summed over the slabs on the host: the words exactly (128 bits), eb in slab order
struct OccTotals {
    std::vector<unsigned __int128> f, q;
    std::vector<double> eb;
    explicit OccTotals(int n) : f((size_t)n, 0), q((size_t)n, 0), eb((size_t)n, 0.0) {}
    void add(const std::vector<double>& host, int n, bool first) {  // one slab's off_host block
        std::vector<unsigned long long> words(4 * (size_t)n);
        std::memcpy(words.data(), host.data(), words.size() * sizeof(unsigned long long));
        for (int i = 0; i < n; ++i) {
            DosWords fw, qw;
            fw.hi = words[i], fw.lo = words[n + i];
            qw.hi = words[2 * n + i], qw.lo = words[3 * n + i];
            f[(size_t)i] += fw.whole();
            q[(size_t)i] += qw.whole();
            eb[(size_t)i] = first ? host[4 * (size_t)n + i] : eb[(size_t)i] + host[4 * (size_t)n + i];
        }
    }
    // x = words / (2^40 NK): the integer is rounded to double once, the division once more
    void finish(int n, double nk_total, double* q_out, double* f_out, double* eb_out) const {
        for (int i = 0; i < n; ++i) {
            f_out[i] = DosWords::to_double(f[(size_t)i]) / nk_total;
            q_out[i] = DosWords::to_double(q[(size_t)i]) / nk_total;
            eb_out[i] = eb[(size_t)i];
        }
    }
};

}  // namespace

extern "C" int tbk_tetra_weights_from_eigenvalues(int device, int dim, const int32_t* mesh, int n_orb, const double* E, double energy, double* w_out) {
    int64_t nk = 0;
    TBK_CHECK(tetra_check_mesh(dim, mesh, OCC_MESH, &nk));
    TBK_ARG(E != nullptr && w_out != nullptr, "E / w is NULL");
    TBK_ARG(n_orb >= 1, "n_orb < 1");
    TBK_ARG(std::isfinite(energy), "the energy is not finite");
    TBK_CHECK(tetra_check_device(device));
    OccPlan L;
    TBK_CHECK(occ_plan(dim, mesh, mesh[0], mesh[0], 0, n_orb, &L));
    TetraOwnedE d_E;
    DevBuf d_w;
    TBK_CHECK(d_E.upload(E, nk, n_orb));
    TBK_CHECK(d_w.reserve(d_E.bytes));
    TBK_CHECK(occ_launch_weights(nullptr, L, d_E.d(), energy, (double)nk, d_w.as<double>()));
    TBK_HIP(hipMemcpy(w_out, d_w.ptr, d_E.bytes, hipMemcpyDeviceToHost));
    return TBK_OK;
}

extern "C" int tbk_occupations_from_eigensystem(int device, int dim, const int32_t* mesh, int n_orb, const double* E, const double* U, double energy,
                                                int64_t k_chunk, double* q_out, double* f_out, double* eb_out) {
    int64_t nk = 0;
    TBK_CHECK(tetra_check_mesh(dim, mesh, OCC_MESH, &nk));
    TBK_ARG(E != nullptr && U != nullptr, "E / U is NULL");
    TBK_ARG(q_out != nullptr && f_out != nullptr && eb_out != nullptr, "q / f / eb is NULL");
    TBK_ARG(n_orb >= 1, "n_orb < 1");
    TBK_ARG(std::isfinite(energy), "the energy is not finite");
    TBK_ARG(k_chunk >= 0, "k_chunk < 0");
    TBK_CHECK(tetra_check_device(device));
    OccPlan L;
    TBK_CHECK(occ_plan(dim, mesh, mesh[0], mesh[0], 0, n_orb, &L));
    const int64_t chunk = k_chunk == 0 ? nk : std::min(k_chunk, nk);
    const size_t u_per_k = (size_t)n_orb * (size_t)n_orb * 2;
    TetraOwnedE d_E;
    DevBuf d_w, d_ws, d_U;
    TBK_CHECK(d_E.upload(E, nk, n_orb));
    TBK_CHECK(d_w.reserve(d_E.bytes));
    TBK_CHECK(d_ws.reserve(L.ws_bytes));
    TBK_CHECK(d_U.reserve((size_t)chunk * u_per_k * sizeof(double)));
    char* ws = d_ws.as<char>();
    TBK_CHECK(occ_launch_weights(nullptr, L, d_E.d(), energy, (double)nk, d_w.as<double>()));
    TBK_CHECK(occ_launch_band(nullptr, L, d_w.as<double>(), d_E.d(), (double)nk, ws));
    TBK_CHECK(occ_clear_buf(nullptr, L, ws));
    for (int64_t c0 = 0; c0 < nk; c0 += chunk) {
        const int64_t nkc = std::min(chunk, nk - c0);
        TBK_HIP(hipMemcpy(d_U.ptr, U + (size_t)c0 * u_per_k, (size_t)nkc * u_per_k * sizeof(double), hipMemcpyHostToDevice));
        TBK_CHECK(occ_launch_contract(nullptr, L, d_U.as<double>(), d_w.as<double>(), c0, nkc, (double)nk, ws));
    }
    TBK_CHECK(occ_launch_reduce(nullptr, L, ws));
    std::vector<double> host(5 * (size_t)n_orb);
    TBK_HIP(hipMemcpy(host.data(), ws + L.off_host, L.host_bytes, hipMemcpyDeviceToHost));
    OccTotals totals(n_orb);
    totals.add(host, n_orb, true);
    totals.finish(n_orb, (double)nk, q_out, f_out, eb_out);
    return TBK_OK;
}

extern "C" int tbk_tetra_weights_multi(tbk_model* const* handles, int n_handles, const int32_t* mesh, double energy, double* w_out) {
    TBK_ARG(w_out != nullptr, "w is NULL");
    TBK_ARG(std::isfinite(energy), "the energy is not finite");
    OccStaged staged;
    TBK_CHECK(staged.make(handles, n_handles, mesh));
    TBK_CHECK(staged.weights(energy, w_out));
    return staged.finish();
}

extern "C" int tbk_tetra_weights(tbk_model* m, const int32_t* mesh, double energy, double* w_out) {
    return tbk_tetra_weights_multi(&m, 1, mesh, energy, w_out);
}

extern "C" int tbk_occupations_multi(tbk_model* const* handles, int n_handles, const int32_t* mesh, int mode, double value, double* mu_out,
                                     double* q_out, double* f_out, double* eb_out) {
    TBK_ARG(mu_out != nullptr && q_out != nullptr && f_out != nullptr && eb_out != nullptr, "mu / q / f / eb is NULL");
    TBK_ARG(mode == 0 || mode == 1, "mode must be 0 (value = energy) or 1 (value = n_electrons)");
    TBK_ARG(handles != nullptr && n_handles >= 1 && handles[0] != nullptr, "no handles");
    if (mode == 1)
        TBK_CHECK(tbk_fermi_check_electrons(value, handles[0]->n_orb));
    else
        TBK_ARG(std::isfinite(value), "the energy is not finite");
    OccStaged staged;
    TBK_CHECK(staged.make(handles, n_handles, mesh));
    TBK_CHECK(staged.find_mu(mesh, mode, value, mu_out));
    TBK_CHECK(staged.weights(mu_out[0], nullptr));
    TBK_CHECK(staged.sums());
    TBK_CHECK(staged.finish());
    OccTotals totals(staged.n_orb);
    for (size_t i = 0; i < staged.occ.size(); ++i) totals.add(staged.occ[i].host, staged.n_orb, i == 0);
    totals.finish(staged.n_orb, (double)staged.nk_total, q_out, f_out, eb_out);
    return TBK_OK;
}

extern "C" int tbk_occupations(tbk_model* m, const int32_t* mesh, int mode, double value, double* mu_out, double* q_out, double* f_out,
                               double* eb_out) {
    return tbk_occupations_multi(&m, 1, mesh, mode, value, mu_out, q_out, f_out, eb_out);
}

extern "C" int tbk_occ_timing(tbk_model* m, double* ms, int64_t* calls, int reset) {
    TBK_ARG(m != nullptr && ms != nullptr && calls != nullptr, "model / ms / calls is NULL");
    return tbk_timed_read(m, TIMED_OCC, 3, ms, calls, nullptr, reset);
}
