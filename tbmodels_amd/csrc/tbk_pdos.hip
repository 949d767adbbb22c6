// tbk_pdos.hip -- the orbital-projected number of states nos_g(E) of a uniform, periodic k mesh by the linear tetrahedron method
// with matrix elements (Bloechl's corner weights; triangles in dim = 2).  Not in the reference; DESIGN.md section 11 has the
// formulas, the layout and the measurements, tools/pdos_model.py is the NumPy statement the tests compare with.
//
//   U[nk][n][n][2]    eigenvectors of one k chunk, U[k][i][b] = component i of band b (tbk_eigh_device, convention 2)
//   W[NK][G][n_orb]   A_g(k, b) = sum_{i in g} |U[k][i][b]|^2 in [0, 1]             (pdos_weights_kernel, per chunk)
//   E[NK][n_orb]      ascending eigenvalues per mesh point, mesh order (last axis fastest)
//   nos[g][j]         = 1 / (S NK) * sum over (cell, band, simplex) of sum_c w_c(E_j) A_g at corner c   (pdos_accumulate_kernel)
//
// The accumulate kernel has the structure of dos_accumulate_kernel (tbk_dos.hip): a work item is one (cell, band) pair, band
// fastest; per simplex the corners are sorted by energy -- adjacent exchanges on a strict comparison, so ties keep corner order,
// and every corner's G weights travel with its energy -- the bins j_lo <= j < j_hi receive sum_c w_c(E_j) A_g,c, the corner
// weights of a (simplex, bin) being computed ONCE and applied to all groups, and the constant every bin from j_hi upwards would
// receive -- the mean of A over the corners, no longer the integer 1 -- is rounded once to fixed point and added at j_hi into a
// per-group step accumulator whose prefix sum comes last.
//
// Reproducibility: as in tbk_dos.hip there are no floating-point atomics.  Contributions in [0, 1] are accumulated in 64-bit
// fixed point (2^-40), every workgroup stores its bins into its own row of a [n_workgroups][G][NE] buffer, the rows are summed
// and the steps prefix-summed in integers: for given E and W the bits of nos depend neither on wave order nor workgroup count.
// Error: a bin of nos_g sums at most S NK n_orb rounded contributions AND at most S NK n_orb rounded steps, each off by at most
// 2^-41, and is divided by S NK: |error| <= 2 n_orb 2^-41 = 9.1e-13 n_orb.
//
// Overflow.  A workgroup takes at most DOS_MAX_ITEMS = 2^20 items, so one of its bins (fraction or step) receives at most
// 6 * 2^20 values of at most 2^40: 6 * 2^60 < 2^64.  The reduction splits every workgroup's bin into its high 44 (< 6 * 2^40) and
// low 20 bits and sums each over at most 2^20 workgroups: < 2^63 and < 2^40.  The prefix sum of the steps would overflow 64 bits
// (up to S NK n_orb terms of 2^40), so it runs on the two halves apart: the high halves of ALL steps sum to at most
// S NK n_orb * 2^20 and the low halves to at most 2^20 bins * 2^40; the launcher refuses S NK n_orb > 2^42 (far beyond what fits
// device memory: NK n_orb (1 + G) doubles), so both stay below 2^63.

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "tbk_tetra_staged.h"

namespace {

constexpr int PDOS_THREADS = 256;
// (group, energy) bins of a workgroup's LDS: a 64-bit fraction and a 64-bit step each = 64 KiB.  The energy tile is
// PDOS_LDS_BINS / GT points for GT = n_groups rounded up to a power of two (the kernel's instantiation): 4096, 2048, ... 256
constexpr int PDOS_LDS_BINS = 4096;
constexpr int64_t PDOS_MAX_TERMS = int64_t(1) << 42;  // S NK n_orb (the overflow bound above)

int pdos_group_tile(int n_groups) {
    int gt = 1;
    while (gt < n_groups) gt *= 2;
    return gt;
}

// ---- eigenvectors -> weights -------------------------------------------------------------------------------------------------
// One thread per (k, band), band fastest: a wave reads 64 consecutive complex numbers of a row of U[k] per orbital.  The groups
// are walked in order, the orbitals of a group in list order; one launch serves all groups, so an element of U comes from HBM
// once (an orbital that sits in several groups is re-read from L2 by the workgroup that just fetched it).
__global__ void __launch_bounds__(PDOS_THREADS) pdos_weights_kernel(const double2* __restrict__ U, int n, int64_t nk, int n_groups,
                                                                    const int32_t* __restrict__ offsets, const int32_t* __restrict__ orbitals,
                                                                    double* __restrict__ W) {
    const int64_t t = (int64_t)blockIdx.x * PDOS_THREADS + threadIdx.x;
    if (t >= nk * n) return;
    const int64_t k = t / n;
    const int b = (int)(t - k * n);
    const double2* Uk = U + (size_t)k * n * n + b;
    double* Wk = W + (size_t)k * n_groups * n + b;
    for (int g = 0; g < n_groups; ++g) {
        double acc = 0.0;
        for (int e = offsets[g]; e < offsets[g + 1]; ++e) {
            const double2 u = Uk[(size_t)orbitals[e] * n];
            acc += u.x * u.x + u.y * u.y;
        }
        Wk[(size_t)g * n] = acc;
    }
}

// ---- accumulate --------------------------------------------------------------------------------------------------------------
// the payload of the stable sort (tbk_tetra.h): every corner's GT weights travel with its energy
template <int GT, int NC>
struct PdosColumns {
    double (&a)[GT][NC];
    template <int A, int B>
    __device__ __forceinline__ void follow(bool sw) {
#pragma unroll
        for (int g = 0; g < GT; ++g) {
            const double x = sw ? a[g][B] : a[g][A], y = sw ? a[g][A] : a[g][B];
            a[g][A] = x;
            a[g][B] = y;
        }
    }
};

// One simplex of NC corners (4: tetrahedron, 3: triangle) whose mesh points are kc[]: DESIGN 11.1.  part / step: [n_groups][tile_n].
// The corner weights of a bin are TetraGaps' (tbk_tetra.h), computed once and applied to all groups.
template <int GT, int NC>
__device__ __forceinline__ void pdos_simplex(const double (&e_in)[NC], const int64_t (&kc)[NC], int band, const double* __restrict__ W,
                                             int n_groups, int n_orb, const DosWindow& w, unsigned long long* part, unsigned long long* step) {
    double e[NC], a[GT][NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) e[c] = e_in[c];
#pragma unroll
    for (int g = 0; g < GT; ++g)
#pragma unroll
        for (int c = 0; c < NC; ++c) a[g][c] = g < n_groups ? W[((size_t)kc[c] * n_groups + g) * n_orb + band] : 0.0;
    PdosColumns<GT, NC> columns{a};
    tetra_stable_sort(e, columns);
    const int j_lo = dos_first_at_or_above(e[0], w.e_min, w.e_step, w.inv_step, w.n_e);
    const int j_hi = dos_first_at_or_above(e[NC - 1], w.e_min, w.e_step, w.inv_step, w.n_e);
    if (j_hi >= w.tile_lo && j_hi < w.tile_lo + w.tile_n) {
#pragma unroll
        for (int g = 0; g < GT; ++g)
            if (g < n_groups) {
                // the mean over the corners, rounded once (exactly 1 for unit weights)
                const double mean = NC == 4 ? 0.25 * (((a[g][0] + a[g][1]) + a[g][2]) + a[g][NC - 1]) : ((a[g][0] + a[g][1]) + a[g][2]) / 3.0;
                atomicAdd(&step[g * w.tile_n + (j_hi - w.tile_lo)], dos_fixed(mean));
            }
    }
    const int lo = max(j_lo, w.tile_lo), hi = min(j_hi, w.tile_lo + w.tile_n);
    if (lo >= hi) return;
    const TetraGaps<NC> gaps(e);
    for (int j = lo; j < hi; ++j) {
        const double E = dos_grid(w.e_min, w.e_step, j);  // e1 <= E < e_top here
        double wc[NC];
        gaps.corner_weights(E, wc);
#pragma unroll
        for (int g = 0; g < GT; ++g)
            if (g < n_groups) {
                double sum = wc[0] * a[g][0] + wc[1] * a[g][1] + wc[2] * a[g][2];
                if constexpr (NC == 4) sum = sum + wc[3] * a[g][3];
                atomicAdd(&part[g * w.tile_n + (j - w.tile_lo)], dos_fixed(sum));
            }
    }
}

// grid: (workgroups, energy tiles).  part_g / step_g: [gridDim.x][n_groups][n_e]; every element is written by exactly one workgroup.
template <int DIM, int GT>
__global__ void __launch_bounds__(PDOS_THREADS)
    pdos_accumulate_kernel(const double* __restrict__ E, const double* __restrict__ W, DosGeom g, int n_groups, double e_min, double e_step,
                           double inv_step, int n_e, unsigned long long* __restrict__ part_g, unsigned long long* __restrict__ step_g) {
    extern __shared__ unsigned long long pdos_lds[];
    constexpr int TILE = PDOS_LDS_BINS / GT;
    DosWindow w;
    w.e_min = e_min;
    w.e_step = e_step;
    w.inv_step = inv_step;
    w.n_e = n_e;
    w.tile_lo = (int)blockIdx.y * TILE;
    w.tile_n = min(TILE, n_e - w.tile_lo);
    const int bins = n_groups * w.tile_n;  // <= PDOS_LDS_BINS
    unsigned long long* part = pdos_lds;   // [n_groups][tile_n]
    unsigned long long* step = pdos_lds + bins;
    const int tid = (int)threadIdx.x;
    for (int t = tid; t < 2 * bins; t += PDOS_THREADS) pdos_lds[t] = 0ull;
    __syncthreads();

    const int64_t first = (int64_t)blockIdx.x * g.items_per_wg;
    const int64_t last = min(first + g.items_per_wg, g.items);
    for (int64_t it = first + tid; it < last; it += PDOS_THREADS) {
        const TetraItem t = tetra_item(g, it);
        const int band = t.band, i0 = t.i0, i1 = t.i1, i2 = t.i2, j0 = t.j0, j1 = t.j1, j2 = t.j2;
        auto at = [&](int a0, int a1, int a2) -> int64_t { return tetra_row(g, a0, a1, a2); };
        auto energy = [&](int64_t k) -> double { return E[k * g.n_orb + band]; };
        if (DIM == 3) {
            // corner k_xyz: x, y, z = step along axis 0, 1, 2
            const int64_t k000 = at(i0, i1, i2), k100 = at(j0, i1, i2), k010 = at(i0, j1, i2), k110 = at(j0, j1, i2);
            const int64_t k001 = at(i0, i1, j2), k101 = at(j0, i1, j2), k011 = at(i0, j1, j2), k111 = at(j0, j1, j2);
            const double c000 = energy(k000), c100 = energy(k100), c010 = energy(k010), c110 = energy(k110);
            const double c001 = energy(k001), c101 = energy(k101), c011 = energy(k011), c111 = energy(k111);
            // the six orders (a, b, c) of the axes: corners 0, e_a, e_a + e_b, e_a + e_b + e_c -- the list of tbk_dos.hip
            const double e012[4] = {c000, c100, c110, c111}, e021[4] = {c000, c100, c101, c111}, e102[4] = {c000, c010, c110, c111};
            const double e120[4] = {c000, c010, c011, c111}, e201[4] = {c000, c001, c101, c111}, e210[4] = {c000, c001, c011, c111};
            const int64_t k012[4] = {k000, k100, k110, k111}, k021[4] = {k000, k100, k101, k111}, k102[4] = {k000, k010, k110, k111};
            const int64_t k120[4] = {k000, k010, k011, k111}, k201[4] = {k000, k001, k101, k111}, k210[4] = {k000, k001, k011, k111};
            pdos_simplex<GT, 4>(e012, k012, band, W, n_groups, g.n_orb, w, part, step);
            pdos_simplex<GT, 4>(e021, k021, band, W, n_groups, g.n_orb, w, part, step);
            pdos_simplex<GT, 4>(e102, k102, band, W, n_groups, g.n_orb, w, part, step);
            pdos_simplex<GT, 4>(e120, k120, band, W, n_groups, g.n_orb, w, part, step);
            pdos_simplex<GT, 4>(e201, k201, band, W, n_groups, g.n_orb, w, part, step);
            pdos_simplex<GT, 4>(e210, k210, band, W, n_groups, g.n_orb, w, part, step);
        } else {
            const int64_t k00 = at(i0, i1, 0), k10 = at(j0, i1, 0), k01 = at(i0, j1, 0), k11 = at(j0, j1, 0);
            const double c00 = energy(k00), c10 = energy(k10), c01 = energy(k01), c11 = energy(k11);
            const double e01[3] = {c00, c10, c11}, e10[3] = {c00, c01, c11};
            const int64_t k01_[3] = {k00, k10, k11}, k10_[3] = {k00, k01, k11};
            pdos_simplex<GT, 3>(e01, k01_, band, W, n_groups, g.n_orb, w, part, step);  // (0, 1)
            pdos_simplex<GT, 3>(e10, k10_, band, W, n_groups, g.n_orb, w, part, step);  // (1, 0)
        }
    }
    __syncthreads();
    const int64_t row = (int64_t)blockIdx.x * n_groups * n_e;
    for (int t = tid; t < bins; t += PDOS_THREADS) {
        const int grp = t / w.tile_n, j = t - grp * w.tile_n;
        const int64_t at_g = row + (int64_t)grp * n_e + w.tile_lo + j;
        part_g[at_g] = part[t];
        step_g[at_g] = step[t];
    }
}

// one thread per (group, bin): the workgroups' rows in index order, in integers, the high and low part of every 64-bit bin apart.
// sums: [4][n_groups * n_e] = fraction high / low, step high / low
__global__ void __launch_bounds__(PDOS_THREADS)
    pdos_reduce_kernel(const unsigned long long* __restrict__ part_g, const unsigned long long* __restrict__ step_g, int n_wg, int64_t n_bins,
                       unsigned long long* __restrict__ sums) {
    const int64_t j = (int64_t)blockIdx.x * PDOS_THREADS + threadIdx.x;
    if (j >= n_bins) return;
    DosWords p, s;
    for (int wg = 0; wg < n_wg; ++wg) {
        p.add(part_g[(int64_t)wg * n_bins + j]);
        s.add(step_g[(int64_t)wg * n_bins + j]);
    }
    sums[j] = p.hi;
    sums[n_bins + j] = p.lo;
    sums[2 * n_bins + j] = s.hi;
    sums[3 * n_bins + j] = s.lo;
}

// one workgroup per group: nos[g][j] = (fraction[j] + sum_{i <= j} step[i]) / denom, the prefix sum on the two halves apart (in
// integers: see Overflow above).  Every thread owns a contiguous segment of the grid.
__global__ void __launch_bounds__(PDOS_THREADS) pdos_scan_kernel(const unsigned long long* __restrict__ sums, int n_e, int64_t n_bins, double denom,
                                                                 double* __restrict__ nos) {
    __shared__ unsigned long long total_hi[PDOS_THREADS], total_lo[PDOS_THREADS];
    const int tid = (int)threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * n_e;
    const unsigned long long* p_hi = sums + base;
    const unsigned long long* p_lo = sums + n_bins + base;
    const unsigned long long* s_hi = sums + 2 * n_bins + base;
    const unsigned long long* s_lo = sums + 3 * n_bins + base;
    const int seg = (n_e + PDOS_THREADS - 1) / PDOS_THREADS;
    const int lo = min(n_e, tid * seg), hi = min(n_e, lo + seg);
    unsigned long long sum_hi = 0, sum_lo = 0;
    for (int j = lo; j < hi; ++j) {
        sum_hi += s_hi[j];
        sum_lo += s_lo[j];
    }
    total_hi[tid] = sum_hi;
    total_lo[tid] = sum_lo;
    __syncthreads();
    unsigned long long run_hi = 0, run_lo = 0;
    for (int t = 0; t < tid; ++t) {
        run_hi += total_hi[t];
        run_lo += total_lo[t];
    }
    for (int j = lo; j < hi; ++j) {
        run_hi += s_hi[j];
        run_lo += s_lo[j];
        DosWords all;  // the low halves carry into the high ones first: the sum of up to 2^20 of them has more than 20 bits
        all.add(run_lo + p_lo[j]);
        all.hi += run_hi + p_hi[j];
        nos[base + j] = all.value() / denom;
    }
}

struct PdosLaunch {
    DosGeom g;
    int n_groups = 0, group_tile = 1, n_wg = 0, n_tiles = 0, n_e = 0;
    size_t off_step = 0, off_sums = 0, ws_bytes = 0;
};

// dim in {2, 3}; cells0 cells along axis 0 out of planes0 planes held in E and W
int pdos_plan(int dim, const int32_t* mesh, int64_t cells0, int64_t planes0, int n_orb, int n_groups, int64_t n_e, PdosLaunch* out) {
    PdosLaunch L;
    L.g = tetra_geom(dim, mesh, cells0, planes0, n_orb);
    TBK_ARG(L.g.items * (dim == 3 ? 6 : 2) <= PDOS_MAX_TERMS, "mesh x orbitals too large for one projected density-of-states call");
    L.n_groups = n_groups;
    L.group_tile = pdos_group_tile(n_groups);
    L.n_e = (int)n_e;
    const int tile = PDOS_LDS_BINS / L.group_tile;
    L.n_tiles = (int)((n_e + tile - 1) / tile);
    // no more rows than 2^24 bins of partials
    const int64_t by_memory = std::max<int64_t>(1, (int64_t(1) << 24) / (n_e * n_groups));
    TBK_CHECK(tetra_partition(L.g.items, PDOS_THREADS, std::min<int64_t>(1024, by_memory),
                              "mesh x orbitals too large for one projected density-of-states call", &L.g.items_per_wg, &L.n_wg));
    const size_t bins = (size_t)n_groups * (size_t)n_e;
    L.off_step = dos_align256((size_t)L.n_wg * bins * sizeof(unsigned long long));
    L.off_sums = 2 * L.off_step;
    L.ws_bytes = L.off_sums + dos_align256(4 * bins * sizeof(unsigned long long));
    *out = L;
    return TBK_OK;
}

template <int DIM>
void pdos_launch_accumulate(hipStream_t s, const PdosLaunch& L, const double* d_E, const double* d_W, double e_min, double e_step,
                            unsigned long long* part_g, unsigned long long* step_g) {
    const int tile = PDOS_LDS_BINS / L.group_tile;
    const size_t lds = (size_t)L.n_groups * (size_t)std::min<int64_t>(L.n_e, tile) * 2 * sizeof(unsigned long long);
    const dim3 grid((unsigned)L.n_wg, (unsigned)L.n_tiles);
#define PDOS_CASE(GT)                                                                                                                     \
    case GT:                                                                                                                              \
        hipLaunchKernelGGL((pdos_accumulate_kernel<DIM, GT>), grid, dim3(PDOS_THREADS), lds, s, d_E, d_W, L.g, L.n_groups, e_min, e_step, \
                           1.0 / e_step, L.n_e, part_g, step_g);                                                                          \
        break;
    switch (L.group_tile) {
        PDOS_CASE(1)
        PDOS_CASE(2)
        PDOS_CASE(4)
        PDOS_CASE(8)
        PDOS_CASE(16)
    }
#undef PDOS_CASE
}

// enqueue: (E, W) -> nos[G][n_e] on stream s (d_ws: L.ws_bytes).  denom = S * NK of the WHOLE mesh.  ev (or NULL): three events,
// in front of the accumulate kernel, behind it, behind the scan
int pdos_launch(hipStream_t s, int dim, const PdosLaunch& L, const double* d_E, const double* d_W, double e_min, double e_step, double denom,
                void* d_ws, double* d_nos, SpanRecorder& timer) {
    static_assert(TBK_PDOS_MAX_GROUPS == 16, "pdos_launch_accumulate instantiates group tiles up to 16");
    char* ws = static_cast<char*>(d_ws);
    auto* part_g = reinterpret_cast<unsigned long long*>(ws);
    auto* step_g = reinterpret_cast<unsigned long long*>(ws + L.off_step);
    auto* sums = reinterpret_cast<unsigned long long*>(ws + L.off_sums);
    const int64_t n_bins = (int64_t)L.n_groups * L.n_e;
    timer.start(1);
    if (dim == 3)
        pdos_launch_accumulate<3>(s, L, d_E, d_W, e_min, e_step, part_g, step_g);
    else
        pdos_launch_accumulate<2>(s, L, d_E, d_W, e_min, e_step, part_g, step_g);
    TBK_HIP(hipGetLastError());
    timer.stop();
    timer.start(2);
    hipLaunchKernelGGL(pdos_reduce_kernel, dim3((unsigned)((n_bins + PDOS_THREADS - 1) / PDOS_THREADS)), dim3(PDOS_THREADS), 0, s, part_g, step_g,
                       L.n_wg, n_bins, sums);
    TBK_HIP(hipGetLastError());
    hipLaunchKernelGGL(pdos_scan_kernel, dim3((unsigned)L.n_groups), dim3(PDOS_THREADS), 0, s, sums, L.n_e, n_bins, denom, d_nos);
    TBK_HIP(hipGetLastError());
    timer.stop();
    return TBK_OK;
}

}  // namespace

// The groups as the C ABI takes them: group g = group_orbitals[group_offsets[g] .. group_offsets[g + 1])
int tbk_pdos_check_groups(int n_orb, const int32_t* group_offsets, const int32_t* group_orbitals, int n_groups) {
    TBK_ARG(group_offsets != nullptr && group_orbitals != nullptr, "group_offsets / group_orbitals is NULL");
    TBK_ARG(n_groups >= 1, "no projection groups");
    TBK_ARG(n_groups <= TBK_PDOS_MAX_GROUPS, "more than TBK_PDOS_MAX_GROUPS projection groups");
    TBK_ARG(group_offsets[0] == 0, "group_offsets[0] must be 0");
    std::vector<char> seen((size_t)std::max(n_orb, 0));
    for (int g = 0; g < n_groups; ++g) {
        TBK_ARG(group_offsets[g + 1] > group_offsets[g], "a projection group is empty");
        TBK_ARG(group_offsets[g + 1] - group_offsets[g] <= n_orb, "an orbital repeats inside a projection group");
        std::fill(seen.begin(), seen.end(), 0);
        for (int32_t e = group_offsets[g]; e < group_offsets[g + 1]; ++e) {
            const int32_t i = group_orbitals[e];
            TBK_ARG(i >= 0 && i < n_orb, "an orbital index of a projection group is out of range");
            TBK_ARG(!seen[(size_t)i], "an orbital repeats inside a projection group");
            seen[(size_t)i] = 1;
        }
    }
    return TBK_OK;
}

// pdos_plan and pdos_launch for a caller that brings weights of its own in [0, 1] (tbk_tdf.hip): the bytes of the workspace, and the
// launch of `cells0` cells out of `planes0` planes on it.  The recorder's stages are pdos_launch's: 1 accumulate, 2 reduction + scan.
int tbk_pdos_weighted_bytes(int dim, const int32_t* mesh, int64_t cells0, int64_t planes0, int n_orb, int n_groups, int64_t n_e, size_t* ws_bytes) {
    PdosLaunch L;
    TBK_CHECK(pdos_plan(dim, mesh, cells0, planes0, n_orb, n_groups, n_e, &L));
    *ws_bytes = L.ws_bytes;
    return TBK_OK;
}

int tbk_pdos_weighted_launch(hipStream_t s, int dim, const int32_t* mesh, int64_t cells0, int64_t planes0, int n_orb, int n_groups, int64_t n_e,
                             const double* d_E, const double* d_W, double e_min, double e_step, double denom, void* d_ws, double* d_nos,
                             SpanRecorder& timer) {
    PdosLaunch L;
    TBK_CHECK(pdos_plan(dim, mesh, cells0, planes0, n_orb, n_groups, n_e, &L));
    return pdos_launch(s, dim, L, d_E, d_W, e_min, e_step, denom, d_ws, d_nos, timer);
}

extern "C" int tbk_pdos_from_eigensystem(int device, int dim, const int32_t* mesh, int n_orb, int n_groups, const double* E, const double* W,
                                         double e_min, double e_step, int64_t n_e, double* nos_out) {
    int64_t nk = 0;
    TBK_CHECK(tbk_dos_check(dim, mesh, e_step, n_e, nos_out, &nk));
    TBK_ARG(E != nullptr && W != nullptr, "E / W is NULL");
    TBK_ARG(n_orb >= 1, "n_orb < 1");
    TBK_ARG(n_groups >= 1 && n_groups <= TBK_PDOS_MAX_GROUPS, "n_groups outside [1, TBK_PDOS_MAX_GROUPS]");
    TBK_ARG(std::isfinite(e_min), "e_min is not finite");
    TBK_CHECK(tetra_check_device(device));
    PdosLaunch L;
    TBK_CHECK(pdos_plan(dim, mesh, mesh[0], mesh[0], n_orb, n_groups, n_e, &L));
    const size_t nos_bytes = (size_t)n_groups * (size_t)n_e * sizeof(double);
    TetraOwnedE d_E;
    DevBuf d_W, d_ws, d_nos;
    TBK_CHECK(d_E.upload(E, nk, n_orb));
    const size_t w_bytes = d_E.bytes * (size_t)n_groups;
    TBK_CHECK(d_W.reserve(w_bytes));
    TBK_CHECK(d_ws.reserve(L.ws_bytes));
    TBK_CHECK(d_nos.reserve(nos_bytes));
    TBK_HIP(hipMemcpy(d_W.ptr, W, w_bytes, hipMemcpyHostToDevice));
    SpanRecorder untimed;
    TBK_CHECK(pdos_launch(nullptr, dim, L, d_E.d(), d_W.as<double>(), e_min, e_step, (double)(dim == 3 ? 6 : 2) * (double)nk, d_ws.ptr,
                          d_nos.as<double>(), untimed));
    TBK_HIP(hipMemcpy(nos_out, d_nos.ptr, nos_bytes, hipMemcpyDeviceToHost));
    return TBK_OK;
}

namespace {

// what one slab keeps between its reservations and its launches
struct PdosSlab {
    PdosLaunch L;
    double* d_W = nullptr;
};

// The reservations of one slab and, enqueued, E and W of its planes: the k list goes through ws_k, E stays in ws_out and W in
// ws_pdos_w (NK n_orb (1 + G) doubles for the planes of the slab and the one periodic neighbour plane its last cells need); the
// eigenvectors exist one k chunk at a time.  E comes from the eigenvector call, so that E and U belong together.
int pdos_fill(const TetraStaged& t, TetraSlab& s, const int32_t* mesh, const int32_t* group_offsets, const int32_t* group_orbitals, int n_groups,
              int64_t n_e, PdosSlab* out) {
    tbk_model* m = s.m;
    const int dim = t.dim, n_orb = t.n_orb;
    const int64_t nk = s.planes * t.plane_pts;
    TBK_CHECK(pdos_plan(dim, mesh, s.p_count, s.planes, n_orb, n_groups, n_e, &out->L));
    TBK_CHECK(tbk_dos_mesh_klist(dim, mesh, s.p_lo, s.planes, &s.h_k));
    const size_t k_bytes = s.h_k.size() * sizeof(double);
    const size_t off_bytes = dos_align256((size_t)(n_groups + 1) * sizeof(int32_t)), orb_bytes = (size_t)group_offsets[n_groups] * sizeof(int32_t);
    const size_t nos_bytes = (size_t)n_groups * (size_t)n_e * sizeof(double);
    // what stays for the whole call first, so that the chunk is chosen from what is left
    TBK_CHECK(m->ws_k.reserve(k_bytes));
    TBK_CHECK(m->ws_out.reserve((size_t)nk * n_orb * sizeof(double)));
    TBK_CHECK(m->ws_pdos_w.reserve((size_t)nk * n_groups * n_orb * sizeof(double)));
    TBK_CHECK(m->ws_pdos_grp.reserve(off_bytes + orb_bytes));
    TBK_CHECK(m->ws_dos.reserve(out->L.ws_bytes + dos_align256(nos_bytes)));
    // k-points per chunk: TBK_OPT_K_CHUNK as given (chunks need not be whole planes nor whole k tiles), else what the eigenvector
    // call itself would take from the free memory -- its U chunk, chunk * n_orb^2 * 16 bytes, is the large term there
    const int64_t chunk = mesh_eigh_chunk(m, nk);
    TBK_CHECK(m->ws_pdos_u.reserve((size_t)chunk * n_orb * n_orb * 2 * sizeof(double)));
    const auto* d_off = m->ws_pdos_grp.as<int32_t>();
    const auto* d_orb = reinterpret_cast<const int32_t*>(m->ws_pdos_grp.as<char>() + off_bytes);
    TBK_HIP(hipMemcpyAsync(m->ws_k.ptr, s.h_k.data(), k_bytes, hipMemcpyHostToDevice, m->stream));
    TBK_HIP(hipMemcpyAsync(m->ws_pdos_grp.ptr, group_offsets, (size_t)(n_groups + 1) * sizeof(int32_t), hipMemcpyHostToDevice, m->stream));
    TBK_HIP(hipMemcpyAsync(m->ws_pdos_grp.as<char>() + off_bytes, group_orbitals, orb_bytes, hipMemcpyHostToDevice, m->stream));

    double* d_E = m->ws_out.as<double>();
    double* d_U = m->ws_pdos_u.as<double>();
    out->d_W = m->ws_pdos_w.as<double>();
    for (int64_t c0 = 0; c0 < nk; c0 += chunk) {
        const int64_t nkc = std::min(chunk, nk - c0);
        TBK_CHECK(tbk_eigh_device(m, m->ws_k.as<double>() + c0 * dim, nkc, 2, nullptr, d_E + c0 * n_orb, d_U));
        s.ev->start(0);
        const int64_t threads = nkc * n_orb;
        hipLaunchKernelGGL(pdos_weights_kernel, dim3((unsigned)((threads + PDOS_THREADS - 1) / PDOS_THREADS)), dim3(PDOS_THREADS), 0, m->stream,
                           reinterpret_cast<const double2*>(d_U), n_orb, nkc, n_groups, d_off, d_orb, out->d_W + (size_t)c0 * n_groups * n_orb);
        TBK_HIP(hipGetLastError());
        s.ev->stop();
    }
    s.d_E = d_E;
    return TBK_OK;
}

}  // namespace

// Cells [p_lo, p_lo + p_count) along axis 0 of the mesh on one handle, a one-slab case of the scaffold (tbk_tetra_staged.h) with
// pdos_fill as its reservation step.  nos_out[G][n_e] -- the caller's, it outlives the wait -- receives this slab's share, already
// divided by S * NK of the whole mesh.  The recorder's stages: 0 the weights kernel, 1 the accumulate kernel, 2 reduction + scan.
int tbk_pdos_slab(tbk_model* m, const int32_t* mesh, int64_t p_lo, int64_t p_count, const int32_t* group_offsets, const int32_t* group_orbitals,
                  int n_groups, double e_min, double e_step, int64_t n_e, double* nos_out) {
    TBK_ARG(m != nullptr, "model is NULL");
    TBK_ARG(!m->kdotp, "a k.p model has no Brillouin zone");
    int64_t nk_total = 0;
    TBK_CHECK(tbk_dos_check(m->dim, mesh, e_step, n_e, nos_out, &nk_total));
    TBK_ARG(std::isfinite(e_min), "e_min is not finite");
    TBK_CHECK(tbk_pdos_check_groups(m->n_orb, group_offsets, group_orbitals, n_groups));
    TBK_ARG(p_lo >= 0 && p_count >= 1 && p_lo + p_count <= mesh[0], "slab outside the mesh");
    PdosSlab own;
    TetraStaged staged;
    TBK_CHECK(staged.make_slab(
        m, mesh, DOS_MESH, p_lo, p_count,
        [&](TetraSlab& s, size_t) { return pdos_fill(staged, s, mesh, group_offsets, group_orbitals, n_groups, n_e, &own); }, true));
    const TetraSlab& s = staged.slabs[0];
    const size_t nos_bytes = (size_t)n_groups * (size_t)n_e * sizeof(double);
    double* d_nos = reinterpret_cast<double*>(m->ws_dos.as<char>() + own.L.ws_bytes);
    TBK_CHECK(pdos_launch(m->stream, staged.dim, own.L, s.d_E, own.d_W, e_min, e_step, (double)(staged.dim == 3 ? 6 : 2) * (double)nk_total,
                          m->ws_dos.ptr, d_nos, *s.ev));
    TBK_HIP(hipMemcpyAsync(nos_out, d_nos, nos_bytes, hipMemcpyDeviceToHost, m->stream));
    return staged.streams.book(TIMED_PDOS, true);
}

extern "C" int tbk_pdos(tbk_model* m, const int32_t* mesh, const int32_t* group_offsets, const int32_t* group_orbitals, int n_groups, double e_min,
                        double e_step, int64_t n_e, double* nos_out) {
    TBK_ARG(m != nullptr, "model is NULL");
    TBK_ARG(mesh != nullptr, "mesh / nos is NULL");
    TBK_ARG(m->dim == 2 || m->dim == 3, DOS_MESH);
    TBK_ARG(mesh[0] >= 1, "a mesh entry is < 1");
    return tbk_pdos_slab(m, mesh, 0, mesh[0], group_offsets, group_orbitals, n_groups, e_min, e_step, n_e, nos_out);
}

extern "C" int tbk_pdos_timing(tbk_model* m, double* ms, int64_t* calls, int reset) {
    TBK_ARG(m != nullptr && ms != nullptr && calls != nullptr, "model / ms / calls is NULL");
    return tbk_timed_read(m, TIMED_PDOS, 3, ms, calls, nullptr, reset);
}
