// tbk_dos.hip -- the number of states nos(E) of a uniform, periodic k mesh by the linear tetrahedron method (dim = 3; triangles in
// dim = 2), from eigenvalues that are already in device memory.  Not in the reference (it has no density of states at all);
// DESIGN.md section 10 has the formulas, the layout and the measurements.
//
//   E[NK][n_orb]   ascending eigenvalues per mesh point, mesh order = np.meshgrid(..., indexing="ij") (last axis fastest)
//   nos[j]         = 1 / (S NK) * sum over (cell, band, simplex) of n_T(E_j),   S = 6 tetrahedra (2 triangles) per cell
//
// A work item is one (cell, band) pair, band fastest: a wave reads 64 consecutive doubles of a row of E per corner.  Per simplex
// the corners are sorted, j_lo = first j with E_j >= e1 and j_hi = first j with E_j >= e_top are found from one multiply (the
// grid is uniform) and settled by the comparison itself, n_T(E_j) is added for j_lo <= j < j_hi only, and the "1" that every
// bin from j_hi upwards would receive is ONE integer count at j_hi: the prefix sum over the counts comes last and is exact.
//
// Reproducibility (include/tbk.h: the same call gives the same bits).  Floating-point atomics add in arrival order, in LDS
// as in global memory, so there are none here: n_T in [0, 1] is accumulated in 64-bit FIXED POINT (integer adds commute), every
// workgroup stores its bins with plain stores into its own row of a [n_workgroups][NE] buffer, and a second kernel sums the rows
// in integers as well.  The result does not depend on the order in which waves run, nor on the number of workgroups.
//
// Bound (measured): VALU issue -- the bin loop of a simplex runs for the longest range among a wave's lanes; the
// reciprocals of the corner gaps are taken once per simplex, so a bin costs FP64 multiplies and adds, no division.

#include <algorithm>
#include <cmath>
#include <vector>

#include "tbk_tetra_staged.h"

namespace {

constexpr int DOS_THREADS = 256;
constexpr int DOS_TILE = 4096;  // energy bins per LDS tile: 4096 * (8 + 4) bytes = 48 KiB; longer grids take gridDim.y tiles
// Fixed point (tbk_tetra.h): a contribution n_T in [0, 1] is stored as round(n_T * 2^40), i.e. with an error of at most 2^-41
// each.  A bin of nos sums at most S NK n_orb of them and is divided by S NK: |error| <= n_orb * 2^-41 = 4.5e-13 n_orb in the worst
// case (every contribution off by half a unit in the same direction), a twentieth of the 1e-11 n_orb the kernel is tested to.
// Overflow: a workgroup takes at most DOS_MAX_ITEMS (cell, band) pairs, so one of its bins receives at most
// 6 * 2^20 contributions of at most 2^40: 6 * 2^60 < 2^64.

// one simplex of NC corners: DESIGN 10.1.  n_T and the reciprocals behind it are TetraGaps' (tbk_tetra.h), taken once per simplex
// and only if the window holds one of its bins: the bin loop has no division
template <int NC>
__device__ __forceinline__ void dos_simplex(const double (&corners)[NC], const DosWindow& w, unsigned long long* part, unsigned* step) {
    double e[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) e[c] = corners[c];
    tetra_sort(e);
    const int j_lo = dos_first_at_or_above(e[0], w.e_min, w.e_step, w.inv_step, w.n_e);
    const int j_hi = dos_first_at_or_above(e[NC - 1], w.e_min, w.e_step, w.inv_step, w.n_e);
    if (j_hi >= w.tile_lo && j_hi < w.tile_lo + w.tile_n) atomicAdd(&step[j_hi - w.tile_lo], 1u);
    const int lo = max(j_lo, w.tile_lo), hi = min(j_hi, w.tile_lo + w.tile_n);
    if (lo >= hi) return;
    const TetraGaps<NC> gaps(e);
    for (int j = lo; j < hi; ++j) {
        const double E = dos_grid(w.e_min, w.e_step, j);  // e1 <= E < e_top here
        atomicAdd(&part[j - w.tile_lo], dos_fixed(gaps.fraction(E)));
    }
}

// grid: (workgroups, energy tiles).  part_g / step_g: [gridDim.x][n_e]; every element is written by exactly one workgroup.
template <int DIM>
__global__ void __launch_bounds__(DOS_THREADS) dos_accumulate_kernel(const double* __restrict__ E, DosGeom g, double e_min, double e_step,
                                                                     double inv_step, int n_e, unsigned long long* __restrict__ part_g,
                                                                     unsigned* __restrict__ step_g) {
    extern __shared__ unsigned long long dos_lds[];
    DosWindow w;
    w.e_min = e_min;
    w.e_step = e_step;
    w.inv_step = inv_step;
    w.n_e = n_e;
    w.tile_lo = (int)blockIdx.y * DOS_TILE;
    w.tile_n = min(DOS_TILE, n_e - w.tile_lo);
    unsigned long long* part = dos_lds;                                 // [tile_n]
    unsigned* step = reinterpret_cast<unsigned*>(dos_lds + w.tile_n);  // [tile_n]
    const int tid = (int)threadIdx.x;
    for (int t = tid; t < w.tile_n; t += DOS_THREADS) {
        part[t] = 0ull;
        step[t] = 0u;
    }
    __syncthreads();

    const int64_t first = (int64_t)blockIdx.x * g.items_per_wg;
    const int64_t last = min(first + g.items_per_wg, g.items);
    for (int64_t it = first + tid; it < last; it += DOS_THREADS) {
        const TetraItem t = tetra_item(g, it);
        const int i0 = t.i0, i1 = t.i1, i2 = t.i2, j0 = t.j0, j1 = t.j1, j2 = t.j2;
        auto at = [&](int a0, int a1, int a2) -> double { return E[tetra_row(g, a0, a1, a2) * g.n_orb + t.band]; };
        if (DIM == 3) {
            // corner c_xyz: x, y, z = step along axis 0, 1, 2
            const double c000 = at(i0, i1, i2), c100 = at(j0, i1, i2), c010 = at(i0, j1, i2), c110 = at(j0, j1, i2);
            const double c001 = at(i0, i1, j2), c101 = at(j0, i1, j2), c011 = at(i0, j1, j2), c111 = at(j0, j1, j2);
            // the six orders (a, b, c) of the axes: corners 0, e_a, e_a + e_b, e_a + e_b + e_c
            dos_simplex<4>({c000, c100, c110, c111}, w, part, step);  // (0, 1, 2)
            dos_simplex<4>({c000, c100, c101, c111}, w, part, step);  // (0, 2, 1)
            dos_simplex<4>({c000, c010, c110, c111}, w, part, step);  // (1, 0, 2)
            dos_simplex<4>({c000, c010, c011, c111}, w, part, step);  // (1, 2, 0)
            dos_simplex<4>({c000, c001, c101, c111}, w, part, step);  // (2, 0, 1)
            dos_simplex<4>({c000, c001, c011, c111}, w, part, step);  // (2, 1, 0)
        } else {
            const double c00 = at(i0, i1, 0), c10 = at(j0, i1, 0), c01 = at(i0, j1, 0), c11 = at(j0, j1, 0);
            dos_simplex<3>({c00, c10, c11}, w, part, step);  // (0, 1)
            dos_simplex<3>({c00, c01, c11}, w, part, step);  // (1, 0)
        }
    }
    __syncthreads();
    const int64_t row = (int64_t)blockIdx.x * n_e + w.tile_lo;
    for (int t = tid; t < w.tile_n; t += DOS_THREADS) {
        part_g[row + t] = part[t];
        step_g[row + t] = step[t];
    }
}

// one thread per bin: the workgroups' rows in index order, in integers (high and low part of every 64-bit bin apart, so that
// neither sum overflows)
__global__ void __launch_bounds__(DOS_THREADS) dos_reduce_kernel(const unsigned long long* __restrict__ part_g, const unsigned* __restrict__ step_g,
                                                                 int n_wg, int n_e, double* __restrict__ frac, long long* __restrict__ count) {
    const int j = (int)blockIdx.x * DOS_THREADS + (int)threadIdx.x;
    if (j >= n_e) return;
    DosWords sum;
    long long c = 0;
    for (int wg = 0; wg < n_wg; ++wg) {
        sum.add(part_g[(int64_t)wg * n_e + j]);
        c += (long long)step_g[(int64_t)wg * n_e + j];
    }
    frac[j] = sum.value();
    count[j] = c;
}

// one workgroup: nos[j] = (frac[j] + sum_{i <= j} count[i]) / denom.  Every thread owns a contiguous segment of the grid.
__global__ void __launch_bounds__(DOS_THREADS) dos_scan_kernel(const double* __restrict__ frac, const long long* __restrict__ count, int n_e,
                                                               double denom, double* __restrict__ nos) {
    __shared__ long long total[DOS_THREADS];
    const int tid = (int)threadIdx.x;
    const int seg = (n_e + DOS_THREADS - 1) / DOS_THREADS;
    const int lo = min(n_e, tid * seg), hi = min(n_e, lo + seg);
    long long sum = 0;
    for (int j = lo; j < hi; ++j) sum += count[j];
    total[tid] = sum;
    __syncthreads();
    long long run = 0;
    for (int t = 0; t < tid; ++t) run += total[t];
    for (int j = lo; j < hi; ++j) {
        run += count[j];
        nos[j] = (frac[j] + (double)run) / denom;
    }
}

struct DosLaunch {
    DosGeom g;
    int n_wg = 0, n_tiles = 0, n_e = 0;
    size_t off_step = 0, off_frac = 0, off_count = 0, ws_bytes = 0;
};

// dim in {2, 3}; cells0 cells along axis 0 out of planes0 planes held in E (planes0 == cells0: the axis wraps onto itself)
int dos_plan(int dim, const int32_t* mesh, int64_t cells0, int64_t planes0, int n_orb, int64_t n_e, DosLaunch* out) {
    DosLaunch L;
    L.g = tetra_geom(dim, mesh, cells0, planes0, n_orb);
    L.n_e = (int)n_e;
    L.n_tiles = (int)((n_e + DOS_TILE - 1) / DOS_TILE);
    // no more rows than 2^24 bins of partials
    const int64_t by_memory = std::max<int64_t>(1, (int64_t(1) << 24) / n_e);
    TBK_CHECK(tetra_partition(L.g.items, DOS_THREADS, std::min<int64_t>(1024, by_memory), "mesh x orbitals too large for one density-of-states call",
                              &L.g.items_per_wg, &L.n_wg));
    const size_t bins = (size_t)L.n_wg * (size_t)n_e;
    L.off_step = dos_align256(bins * sizeof(unsigned long long));
    L.off_frac = L.off_step + dos_align256(bins * sizeof(unsigned));
    L.off_count = L.off_frac + dos_align256((size_t)n_e * sizeof(double));
    L.ws_bytes = L.off_count + dos_align256((size_t)n_e * sizeof(long long));
    *out = L;
    return TBK_OK;
}

// enqueue: E -> nos on stream s (d_ws: L.ws_bytes).  denom = S * NK of the WHOLE mesh.
int dos_launch(hipStream_t s, int dim, const DosLaunch& L, const double* d_E, double e_min, double e_step, double denom, void* d_ws,
               double* d_nos) {
    char* ws = static_cast<char*>(d_ws);
    auto* part_g = reinterpret_cast<unsigned long long*>(ws);
    auto* step_g = reinterpret_cast<unsigned*>(ws + L.off_step);
    auto* frac = reinterpret_cast<double*>(ws + L.off_frac);
    auto* count = reinterpret_cast<long long*>(ws + L.off_count);
    const size_t lds = (size_t)std::min<int64_t>(L.n_e, DOS_TILE) * (sizeof(unsigned long long) + sizeof(unsigned));
    const dim3 grid((unsigned)L.n_wg, (unsigned)L.n_tiles);
    if (dim == 3)
        hipLaunchKernelGGL(dos_accumulate_kernel<3>, grid, dim3(DOS_THREADS), lds, s, d_E, L.g, e_min, e_step, 1.0 / e_step, L.n_e, part_g, step_g);
    else
        hipLaunchKernelGGL(dos_accumulate_kernel<2>, grid, dim3(DOS_THREADS), lds, s, d_E, L.g, e_min, e_step, 1.0 / e_step, L.n_e, part_g, step_g);
    TBK_HIP(hipGetLastError());
    hipLaunchKernelGGL(dos_reduce_kernel, dim3((unsigned)((L.n_e + DOS_THREADS - 1) / DOS_THREADS)), dim3(DOS_THREADS), 0, s, part_g, step_g,
                       L.n_wg, L.n_e, frac, count);
    TBK_HIP(hipGetLastError());
    hipLaunchKernelGGL(dos_scan_kernel, dim3(1), dim3(DOS_THREADS), 0, s, frac, count, L.n_e, denom, d_nos);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

}  // namespace

// ---- what the four tetrahedron files share on the host (tbk_tetra.h) ---------------------------------------------------------------
int tetra_check_mesh(int dim, const int32_t* mesh, const char* what, int64_t* nk_total) {
    TBK_ARG(dim == 2 || dim == 3, what);
    TBK_ARG(mesh != nullptr, "mesh is NULL");
    int64_t nk = 1;
    for (int d = 0; d < dim; ++d) {
        TBK_ARG(mesh[d] >= 1, "a mesh entry is < 1");
        nk *= mesh[d];
        TBK_ARG(nk < (int64_t(1) << 31), "the mesh has 2^31 points or more");
    }
    *nk_total = nk;
    return TBK_OK;
}

int tbk_dos_check(int dim, const int32_t* mesh, double e_step, int64_t n_e, const void* nos_out, int64_t* nk_total) {
    if (dim == 2 || dim == 3) TBK_ARG(mesh != nullptr && nos_out != nullptr, "mesh / nos is NULL");  // (a wrong dim is reported first)
    TBK_CHECK(tetra_check_mesh(dim, mesh, DOS_MESH, nk_total));
    TBK_ARG(n_e >= 2, "the energy grid needs at least two points");
    TBK_ARG(n_e <= DOS_MAX_NE, "the energy grid has more than 2^20 points");
    TBK_ARG(std::isfinite(e_step) && e_step > 0.0, "the energy step must be positive and finite");
    return TBK_OK;
}

int tetra_check_device(int device) {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0) {
        (void)hipGetLastError();
        tbk_set_error("no HIP device visible: libtbk has no CPU path");
        return TBK_ERR_DEVICE;
    }
    TBK_ARG(device >= 0 && device < n_dev, "device out of range");
    TBK_HIP(hipSetDevice(device));
    return TBK_OK;
}

DosGeom tetra_geom(int dim, const int32_t* mesh, int64_t cells0, int64_t planes0, int n_orb) {
    DosGeom g;
    g.n0_cells = (int)cells0;
    g.n0_planes = (int)planes0;
    g.n1 = mesh[1];
    g.n2 = dim == 3 ? mesh[2] : 1;
    g.n_orb = n_orb;
    g.items = cells0 * g.n1 * g.n2 * n_orb;
    g.items_per_wg = 0;
    return g;
}

int tetra_partition(int64_t items, int threads, int64_t cap, const char* what, int64_t* items_per_wg, int* n_wg_out) {
    int64_t n_wg = std::min<int64_t>((items + threads - 1) / threads, cap);
    n_wg = std::max<int64_t>(n_wg, (items + DOS_MAX_ITEMS - 1) / DOS_MAX_ITEMS);
    TBK_ARG(n_wg <= (int64_t(1) << DOS_SPLIT_BITS), what);
    *items_per_wg = (items + n_wg - 1) / n_wg;
    *n_wg_out = (int)((items + *items_per_wg - 1) / *items_per_wg);
    return TBK_OK;
}

int TetraHandles::open(tbk_model* const* handles, int n_handles, const int32_t* mesh, const char* what) {
    TBK_ARG(handles != nullptr && n_handles >= 1, "no handles");
    for (int i = 0; i < n_handles; ++i) {
        TBK_ARG(handles[i] != nullptr, "a handle is NULL");
        TBK_ARG(handles[i]->dim == handles[0]->dim && handles[i]->n_orb == handles[0]->n_orb, "handles of different models (dim / n_orb differ)");
        TBK_ARG(!handles[i]->kdotp, "a k.p model has no Brillouin zone");
    }
    std::vector<tbk_model*> order(handles, handles + n_handles);
    std::sort(order.begin(), order.end());
    order.erase(std::unique(order.begin(), order.end()), order.end());
    TBK_ARG((int)order.size() == n_handles, "a handle appears twice");
    dim = handles[0]->dim;
    n_orb = handles[0]->n_orb;
    TBK_CHECK(tetra_check_mesh(dim, mesh, what, &nk_total));
    plane_pts = nk_total / mesh[0];
    cut = TetraSlabs(mesh[0], n_handles);
    for (tbk_model* m : order) locks.emplace_back(m->mu);
    return TBK_OK;
}

// the k list of `planes` planes of axis 0 from plane p_lo on, in mesh order (the order tbk_fold.hip recognises): k_d = i_d / n_d
int tbk_dos_mesh_klist(int dim, const int32_t* mesh, int64_t p_lo, int64_t planes, std::vector<double>* h_k) {
    const int64_t n0 = mesh[0];
    const int n1 = mesh[1], n2 = dim == 3 ? mesh[2] : 1;
    try {
        h_k->resize((size_t)(planes * n1 * n2) * dim);
    } catch (...) {
        tbk_set_error("cannot allocate the k list of the mesh");
        return TBK_ERR_MEMORY;
    }
    size_t q = 0;
    for (int64_t p = 0; p < planes; ++p) {
        const double k0 = (double)((p_lo + p) % n0) / (double)n0;
        for (int i1 = 0; i1 < n1; ++i1) {
            const double k1 = (double)i1 / (double)n1;
            for (int i2 = 0; i2 < n2; ++i2) {
                (*h_k)[q++] = k0;
                (*h_k)[q++] = k1;
                if (dim == 3) (*h_k)[q++] = (double)i2 / (double)n2;
            }
        }
    }
    return TBK_OK;
}

int tbk_mesh_eigenvalues(tbk_model* m, const int32_t* mesh, int64_t p_lo, int64_t planes, bool below, std::vector<double>* h_k) {
    const int dim = m->dim, n_orb = m->n_orb;
    const int64_t n0 = mesh[0], plane_pts = (int64_t)mesh[1] * (dim == 3 ? mesh[2] : 1);
    TBK_CHECK(tbk_dos_mesh_klist(dim, mesh, p_lo, planes, h_k));
    if (below) {
        std::vector<double> head;
        TBK_CHECK(tbk_dos_mesh_klist(dim, mesh, (p_lo - 1 + n0) % n0, 1, &head));
        try {
            h_k->insert(h_k->begin(), head.begin(), head.end());
        } catch (...) {
            tbk_set_error("cannot allocate the k list of the mesh");
            return TBK_ERR_MEMORY;
        }
    }
    const int64_t head_pts = below ? plane_pts : 0, nk = planes * plane_pts;
    const size_t k_bytes = h_k->size() * sizeof(double);
    TBK_CHECK(m->ws_k.reserve(k_bytes));
    TBK_CHECK(m->ws_out.reserve((size_t)(head_pts + nk) * n_orb * sizeof(double)));
    TBK_HIP(hipMemcpyAsync(m->ws_k.ptr, h_k->data(), k_bytes, hipMemcpyHostToDevice, m->stream));
    TBK_CHECK(tbk_eigenval_device_hint(m, m->ws_k.as<double>() + head_pts * dim, h_k->data() + head_pts * dim, nk,
                                       m->ws_out.as<double>() + head_pts * n_orb));
    if (below) TBK_CHECK(tbk_eigenval_device_hint(m, m->ws_k.as<double>(), h_k->data(), plane_pts, m->ws_out.as<double>()));
    return TBK_OK;
}

extern "C" int tbk_dos_from_eigenvalues(int device, int dim, const int32_t* mesh, int n_orb, const double* E, double e_min, double e_step,
                                        int64_t n_e, double* nos_out) {
    int64_t nk = 0;
    TBK_CHECK(tbk_dos_check(dim, mesh, e_step, n_e, nos_out, &nk));
    TBK_ARG(E != nullptr, "E is NULL");
    TBK_ARG(n_orb >= 1, "n_orb < 1");
    TBK_ARG(std::isfinite(e_min), "e_min is not finite");
    TBK_CHECK(tetra_check_device(device));
    DosLaunch L;
    TBK_CHECK(dos_plan(dim, mesh, mesh[0], mesh[0], n_orb, n_e, &L));
    TetraOwnedE d_E;
    DevBuf d_ws, d_nos;
    TBK_CHECK(d_E.upload(E, nk, n_orb));
    TBK_CHECK(d_ws.reserve(L.ws_bytes));
    TBK_CHECK(d_nos.reserve((size_t)n_e * sizeof(double)));
    TBK_CHECK(dos_launch(nullptr, dim, L, d_E.d(), e_min, e_step, (double)(dim == 3 ? 6 : 2) * (double)nk, d_ws.ptr, d_nos.as<double>()));
    TBK_HIP(hipMemcpy(nos_out, d_nos.ptr, (size_t)n_e * sizeof(double), hipMemcpyDeviceToHost));
    return TBK_OK;
}

// Cells [p_lo, p_lo + p_count) along axis 0 of the mesh on one handle, a one-slab case of the scaffold (tbk_tetra_staged.h): the
// eigenvalues of those planes and of the one periodic neighbour plane the last cells need (none when the slab is the whole axis)
// stay in HBM; nos_out -- the caller's, it outlives the wait -- receives this slab's share of nos, already divided by S * NK of
// the whole mesh.
int tbk_dos_slab(tbk_model* m, const int32_t* mesh, int64_t p_lo, int64_t p_count, double e_min, double e_step, int64_t n_e, double* nos_out) {
    TBK_ARG(m != nullptr, "model is NULL");
    TBK_ARG(!m->kdotp, "a k.p model has no Brillouin zone");
    int64_t nk_total = 0;
    TBK_CHECK(tbk_dos_check(m->dim, mesh, e_step, n_e, nos_out, &nk_total));
    TBK_ARG(std::isfinite(e_min), "e_min is not finite");
    TBK_ARG(p_lo >= 0 && p_count >= 1 && p_lo + p_count <= mesh[0], "slab outside the mesh");
    DosLaunch L;
    TetraStaged staged;
    TBK_CHECK(staged.make_slab(
        m, mesh, DOS_MESH, p_lo, p_count,
        [&](TetraSlab& s, size_t) -> int {
            TBK_CHECK(dos_plan(staged.dim, mesh, s.p_count, s.planes, staged.n_orb, n_e, &L));
            return m->ws_dos.reserve(L.ws_bytes + dos_align256((size_t)n_e * sizeof(double)));
        },
        false));
    const TetraSlab& s = staged.slabs[0];
    double* d_nos = reinterpret_cast<double*>(m->ws_dos.as<char>() + L.ws_bytes);
    s.ev->start();
    TBK_CHECK(dos_launch(m->stream, staged.dim, L, s.d_E, e_min, e_step, (double)(staged.dim == 3 ? 6 : 2) * (double)nk_total, m->ws_dos.ptr, d_nos));
    s.ev->stop();
    TBK_HIP(hipMemcpyAsync(nos_out, d_nos, (size_t)n_e * sizeof(double), hipMemcpyDeviceToHost, m->stream));
    return staged.streams.book(TIMED_DOS, true);
}

extern "C" int tbk_dos(tbk_model* m, const int32_t* mesh, double e_min, double e_step, int64_t n_e, double* nos_out) {
    TBK_ARG(m != nullptr, "model is NULL");
    TBK_ARG(mesh != nullptr, "mesh / nos is NULL");
    TBK_ARG(m->dim == 2 || m->dim == 3, DOS_MESH);
    TBK_ARG(mesh[0] >= 1, "a mesh entry is < 1");
    return tbk_dos_slab(m, mesh, 0, mesh[0], e_min, e_step, n_e, nos_out);
}

extern "C" int tbk_dos_timing(tbk_model* m, double* ms, int64_t* calls, int reset) {
    TBK_ARG(m != nullptr && ms != nullptr && calls != nullptr, "model / ms / calls is NULL");
    return tbk_timed_read(m, TIMED_DOS, 1, ms, calls, nullptr, reset);
}
