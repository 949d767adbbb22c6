// tbk_fermi.hip -- the number of states N(E) of a uniform, periodic k mesh at a handful of ARBITRARY energies, the per-band minimum
// and maximum over the mesh, and the Fermi level for n electrons per cell: a search on doubles that refines a bracket with the
// first kernel until it is one double wide.  Not in the reference; DESIGN.md section 12 has the quantities, the comparison rule
// and the measurements, tools/fermi_model.py is the exact statement the tests compare with.
//
//   E[NK][n_orb]    ascending eigenvalues per mesh point, mesh order (last axis fastest): what tbk_dos.hip reads
//   N(E_m)          = Q(E_m) / (2^40 S NK),  Q(E) = sum over (cell, band, simplex) of round(n_T(E) 2^40) for e1 <= E < e_top
//                                                   + 2^40 * (number of simplices with e_top <= E)
//
// nos_probe_kernel has the work partition and the corner loads of dos_accumulate_kernel (tbk_dos.hip): a work item is one
// (cell, band) pair, band fastest, a wave reads 64 consecutive doubles per corner.  There is no energy grid, no search on one and no
// LDS bins: the up to 16 probe energies are kernel arguments, and every thread keeps one 64-bit fixed-point sum and one count per
// probe in registers (every loop over the probes is unrolled; no accumulator is indexed dynamically).  Per simplex the corners are
// sorted, count[m] += (E_m >= e_top), and n_T is evaluated for the probes with e1 <= E_m < e_top only; the six reciprocals of the
// scaled corner gaps are taken once per simplex and only if some probe of the wave's lanes needs them.  The sort and n_T are
// those of dos_simplex: tetra_sort and TetraGaps::fraction (tbk_tetra.h).
//
// Reproducibility.  No floating-point sum crosses a thread: the wave adds its lanes' integers with shuffles, the workgroup adds its
// waves' with integer LDS atomics, every workgroup stores its row [16] with plain stores, and a second kernel sums the rows, the
// high 44 and low 20 bits of every 64-bit sum apart (DosWords, tbk_tetra.h).  Per probe the result is the exact integer triple
// (count, high, low): independent of wave order, of the workgroup count and of which other probes shared the launch.
// Overflow: the bound of tbk_dos.hip -- a workgroup takes at most DOS_MAX_ITEMS items, so one of its sums is below 6 * 2^60.
//
// band_edges_kernel: min / max per band over the mesh rows.  Both are order independent, so fmin / fmax partials per workgroup and
// a second step give the same bits whatever the launch shape.

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "tbk_tetra_staged.h"

namespace {

constexpr int FERMI_THREADS = 256;
constexpr int FERMI_SEARCH_M = 15;    // probes per pass of the search: 16 sub-intervals, 4 bits of the ordered image per pass
constexpr int FERMI_EDGE_WG = 256;    // row workgroups of the band-edge kernel, at most

struct FermiProbes {
    double e[FERMI_PROBES];
};

// one simplex of NC corners at every probe: count[m] += (E_m >= e_top), frac[m] += n_T(E_m) for e1 <= E_m < e_top
template <int NC>
__device__ __forceinline__ void fermi_simplex(const double (&corners)[NC], const FermiProbes& p, unsigned long long (&frac)[FERMI_PROBES],
                                              unsigned (&count)[FERMI_PROBES]) {
    double e[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) e[c] = corners[c];
    tetra_sort(e);
    bool inside = false;
#pragma unroll
    for (int m = 0; m < FERMI_PROBES; ++m) {
        count[m] += p.e[m] >= e[NC - 1] ? 1u : 0u;
        inside = inside || (p.e[m] >= e[0] && p.e[m] < e[NC - 1]);
    }
    if (!inside) return;
    const TetraGaps<NC> gaps(e);
#pragma unroll
    for (int m = 0; m < FERMI_PROBES; ++m) {
        const double E = p.e[m];
        if (E >= e[0] && E < e[NC - 1]) frac[m] += dos_fixed(gaps.fraction(E));
    }
}

// grid: workgroups.  part_g / count_g: [gridDim.x][FERMI_PROBES]; every element is written by exactly one workgroup.  Probe slots
// the caller does not use repeat its last energy.
template <int DIM>
__global__ void __launch_bounds__(FERMI_THREADS) nos_probe_kernel(const double* __restrict__ E, DosGeom g, FermiProbes p,
                                                                  unsigned long long* __restrict__ part_g, unsigned* __restrict__ count_g) {
    __shared__ unsigned long long wg_frac[FERMI_PROBES];
    __shared__ unsigned wg_count[FERMI_PROBES];
    const int tid = (int)threadIdx.x;
    if (tid < FERMI_PROBES) {
        wg_frac[tid] = 0ull;
        wg_count[tid] = 0u;
    }
    __syncthreads();
    unsigned long long frac[FERMI_PROBES];
    unsigned count[FERMI_PROBES];
#pragma unroll
    for (int m = 0; m < FERMI_PROBES; ++m) {
        frac[m] = 0ull;
        count[m] = 0u;
    }

    const int64_t first = (int64_t)blockIdx.x * g.items_per_wg;
    const int64_t last = min(first + g.items_per_wg, g.items);
    for (int64_t it = first + tid; it < last; it += FERMI_THREADS) {
        const TetraItem t = tetra_item(g, it);
        const int i0 = t.i0, i1 = t.i1, i2 = t.i2, j0 = t.j0, j1 = t.j1, j2 = t.j2;
        auto at = [&](int a0, int a1, int a2) -> double { return E[tetra_row(g, a0, a1, a2) * g.n_orb + t.band]; };
        if (DIM == 3) {
            // corner c_xyz: x, y, z = step along axis 0, 1, 2
            const double c000 = at(i0, i1, i2), c100 = at(j0, i1, i2), c010 = at(i0, j1, i2), c110 = at(j0, j1, i2);
            const double c001 = at(i0, i1, j2), c101 = at(j0, i1, j2), c011 = at(i0, j1, j2), c111 = at(j0, j1, j2);
            // the six orders (a, b, c) of the axes: corners 0, e_a, e_a + e_b, e_a + e_b + e_c -- the list of tbk_dos.hip.  A loop
            // that is not unrolled, so that the probe code exists once: the two middle corners are selected by a uniform index
#pragma unroll 1
            for (int s = 0; s < 6; ++s) {
                const double ca = s < 2 ? c100 : s < 4 ? c010 : c001;
                const double cb = s == 0 || s == 2 ? c110 : s == 1 || s == 4 ? c101 : c011;
                fermi_simplex<4>({c000, ca, cb, c111}, p, frac, count);
            }
        } else {
            const double c00 = at(i0, i1, 0), c10 = at(j0, i1, 0), c01 = at(i0, j1, 0), c11 = at(j0, j1, 0);
#pragma unroll 1
            for (int s = 0; s < 2; ++s) fermi_simplex<3>({c00, s == 0 ? c10 : c01, c11}, p, frac, count);
        }
    }
    // the workgroup's sums, in integers: across the wave with shuffles, across the waves with LDS integer atomics
#pragma unroll
    for (int m = 0; m < FERMI_PROBES; ++m) {
        unsigned long long f = frac[m];
        unsigned n = count[m];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            f += __shfl_xor(f, off);
            n += __shfl_xor(n, off);
        }
        if ((tid & 63) == 0) {
            atomicAdd(&wg_frac[m], f);
            atomicAdd(&wg_count[m], n);
        }
    }
    __syncthreads();
    if (tid < FERMI_PROBES) {
        part_g[(int64_t)blockIdx.x * FERMI_PROBES + tid] = wg_frac[tid];
        count_g[(int64_t)blockIdx.x * FERMI_PROBES + tid] = wg_count[tid];
    }
}

// one workgroup: 16 row lanes per probe walk the workgroups' rows, the high and low part of every 64-bit sum apart (neither sum
// overflows up to 2^20 rows), and meet in integer LDS atomics.  sums[m] = {count, high, low}
__global__ void __launch_bounds__(FERMI_THREADS) nos_probe_reduce_kernel(const unsigned long long* __restrict__ part_g,
                                                                         const unsigned* __restrict__ count_g, int n_wg,
                                                                         unsigned long long* __restrict__ sums) {
    __shared__ unsigned long long total[FERMI_PROBES * 3];
    const int tid = (int)threadIdx.x;
    if (tid < FERMI_PROBES * 3) total[tid] = 0ull;
    __syncthreads();
    const int m = tid % FERMI_PROBES;
    DosWords sum;
    unsigned long long c = 0;
    for (int wg = tid / FERMI_PROBES; wg < n_wg; wg += FERMI_THREADS / FERMI_PROBES) {
        sum.add(part_g[(int64_t)wg * FERMI_PROBES + m]);
        c += (unsigned long long)count_g[(int64_t)wg * FERMI_PROBES + m];
    }
    atomicAdd(&total[m * 3 + 0], c);
    atomicAdd(&total[m * 3 + 1], sum.hi);
    atomicAdd(&total[m * 3 + 2], sum.lo);
    __syncthreads();
    if (tid < FERMI_PROBES * 3) sums[tid] = total[tid];
}

// Per-band minimum and maximum over `rows` rows of E[rows][n_orb].  Up to 256 orbitals a workgroup reads 256 / n_orb whole rows per
// step (contiguous doubles; a thread keeps its band), above that grid.y walks the bands in blocks of 256.  grid.x workgroups share
// the rows; pmin / pmax: [gridDim.x][n_orb].
__global__ void __launch_bounds__(FERMI_THREADS) band_edges_kernel(const double* __restrict__ E, int64_t rows, int n_orb,
                                                                   double* __restrict__ pmin, double* __restrict__ pmax) {
    __shared__ double s_min[FERMI_THREADS], s_max[FERMI_THREADS];
    const int tid = (int)threadIdx.x;
    const int per_step = n_orb <= FERMI_THREADS ? FERMI_THREADS / n_orb : 1;  // rows per step
    const int width = n_orb <= FERMI_THREADS ? n_orb : min(FERMI_THREADS, n_orb - (int)blockIdx.y * FERMI_THREADS);
    const int lane_row = tid / width, lane_band = tid - lane_row * width;
    const int band = (int)blockIdx.y * FERMI_THREADS + lane_band;
    double lo = INFINITY, hi = -INFINITY;
    if (lane_row < per_step) {
        for (int64_t r = (int64_t)blockIdx.x * per_step + lane_row; r < rows; r += (int64_t)gridDim.x * per_step) {
            const double e = E[r * n_orb + band];
            lo = fmin(lo, e);
            hi = fmax(hi, e);
        }
    }
    s_min[tid] = lo;
    s_max[tid] = hi;
    __syncthreads();
    if (tid < width) {
        for (int q = 1; q < per_step; ++q) {
            lo = fmin(lo, s_min[q * width + tid]);
            hi = fmax(hi, s_max[q * width + tid]);
        }
        pmin[(int64_t)blockIdx.x * n_orb + band] = lo;
        pmax[(int64_t)blockIdx.x * n_orb + band] = hi;
    }
}

// one thread per band over the workgroups' partials
__global__ void __launch_bounds__(FERMI_THREADS) band_edges_reduce_kernel(const double* __restrict__ pmin, const double* __restrict__ pmax, int n_wg,
                                                                          int n_orb, double* __restrict__ emin, double* __restrict__ emax) {
    const int band = (int)blockIdx.x * FERMI_THREADS + (int)threadIdx.x;
    if (band >= n_orb) return;
    double lo = INFINITY, hi = -INFINITY;
    for (int wg = 0; wg < n_wg; ++wg) {
        lo = fmin(lo, pmin[(int64_t)wg * n_orb + band]);
        hi = fmax(hi, pmax[(int64_t)wg * n_orb + band]);
    }
    emin[band] = lo;
    emax[band] = hi;
}

// ---- host: one slab of the mesh on one device (FermiLaunch, FermiSlab: tbk_tetra_staged.h) --------------------------------------

// dim in {2, 3}; cells0 cells along axis 0 out of planes0 planes held in E
int fermi_plan(int dim, const int32_t* mesh, int64_t cells0, int64_t planes0, int n_orb, FermiLaunch* out) {
    FermiLaunch L;
    L.g = tetra_geom(dim, mesh, cells0, planes0, n_orb);
    L.rows = L.g.items / n_orb;
    TBK_CHECK(tetra_partition(L.g.items, FERMI_THREADS, 1024, "mesh x orbitals too large for one Fermi-level call", &L.g.items_per_wg, &L.n_wg));
    const int per_step = n_orb <= FERMI_THREADS ? FERMI_THREADS / n_orb : 1;
    L.edge_wg = (int)std::min<int64_t>(FERMI_EDGE_WG, (L.rows + per_step - 1) / per_step);
    L.off_count = dos_align256((size_t)L.n_wg * FERMI_PROBES * sizeof(unsigned long long));
    L.off_sums = L.off_count + dos_align256((size_t)L.n_wg * FERMI_PROBES * sizeof(unsigned));
    L.off_pmin = L.off_sums + dos_align256((size_t)FERMI_PROBES * 3 * sizeof(unsigned long long));
    const size_t partial = dos_align256((size_t)L.edge_wg * (size_t)n_orb * sizeof(double)), edge = dos_align256((size_t)n_orb * sizeof(double));
    L.off_pmax = L.off_pmin + partial;
    L.off_emin = L.off_pmax + partial;
    L.off_emax = L.off_emin + edge;
    L.ws_bytes = L.off_emax + edge;
    *out = L;
    return TBK_OK;
}

// Q(E) of include/tbk.h as (whole, rem): Q = whole * 2^40 + rem, rem < 2^40.  Sums of them are exact.
struct FermiCount {
    unsigned long long whole = 0, rem = 0;
    void add(const FermiCount& o) {
        rem += o.rem;
        whole += o.whole + (rem >> DOS_FRAC_BITS);
        rem &= (1ull << DOS_FRAC_BITS) - 1;
    }
    bool at_least(const FermiCount& t) const { return whole > t.whole || (whole == t.whole && rem >= t.rem); }
};

FermiCount fermi_count(const unsigned long long* triple) {  // {count, high, low} of nos_probe_reduce_kernel
    DosWords sum;
    sum.hi = triple[1];
    sum.lo = triple[2];
    const unsigned __int128 v = sum.whole();
    FermiCount q;
    q.whole = triple[0] + (unsigned long long)(v >> DOS_FRAC_BITS);
    q.rem = (unsigned long long)(v & (((unsigned __int128)1 << DOS_FRAC_BITS) - 1));
    return q;
}

// N = Q / (2^40 simplices): the 86-bit integer is rounded to double once, the division once more
double fermi_nos(const FermiCount& q, int64_t simplices) {
    return DosWords::to_double(((unsigned __int128)q.whole << DOS_FRAC_BITS) + q.rem) / (double)simplices;
}

// the smallest integer >= n_electrons * simplices * 2^40 (n_electrons > 0 finite, simplices < 2^34): Q >= t  <=>  Q >= ceil(t)
FermiCount fermi_target(double n_electrons, int64_t simplices) {
    int exp2 = 0;
    const double mant = std::frexp(n_electrons, &exp2);  // n = mant * 2^exp2, mant in [0.5, 1)
    const unsigned __int128 prod = (unsigned __int128)(unsigned long long)std::ldexp(mant, 53) * (unsigned __int128)(unsigned long long)simplices;
    const int shift = exp2 - 53 + DOS_FRAC_BITS;  // t = prod * 2^shift, prod < 2^87
    unsigned __int128 t;
    if (shift >= 0)
        t = prod << shift;  // n < n_orb <= 2^12: t < 2^86
    else if (-shift >= 127)
        t = 1;
    else
        t = (prod >> -shift) + ((prod & (((unsigned __int128)1 << -shift) - 1)) != 0 ? 1 : 0);
    FermiCount q;
    q.whole = (unsigned long long)(t >> DOS_FRAC_BITS);
    q.rem = (unsigned long long)(t & (((unsigned __int128)1 << DOS_FRAC_BITS) - 1));
    return q;
}

// enqueue: N at n probes (1 .. 16) of this slab's cells -> h_sums, behind the stream
int fermi_probe_enqueue(FermiSlab& s, const double* energies, int n) {
    FermiProbes p;
    for (int m = 0; m < FERMI_PROBES; ++m) p.e[m] = energies[std::min(m, n - 1)];
    TBK_HIP(hipSetDevice(s.device));
    auto* part_g = reinterpret_cast<unsigned long long*>(s.d_ws);
    auto* count_g = reinterpret_cast<unsigned*>(s.d_ws + s.L.off_count);
    auto* sums = reinterpret_cast<unsigned long long*>(s.d_ws + s.L.off_sums);
    if (s.ev) s.ev->start();
    if (s.dim == 3)
        hipLaunchKernelGGL(nos_probe_kernel<3>, dim3((unsigned)s.L.n_wg), dim3(FERMI_THREADS), 0, s.stream, s.d_E, s.L.g, p, part_g, count_g);
    else
        hipLaunchKernelGGL(nos_probe_kernel<2>, dim3((unsigned)s.L.n_wg), dim3(FERMI_THREADS), 0, s.stream, s.d_E, s.L.g, p, part_g, count_g);
    TBK_HIP(hipGetLastError());
    hipLaunchKernelGGL(nos_probe_reduce_kernel, dim3(1), dim3(FERMI_THREADS), 0, s.stream, part_g, count_g, s.L.n_wg, sums);
    TBK_HIP(hipGetLastError());
    if (s.ev) s.ev->stop();
    TBK_HIP(hipMemcpyAsync(s.h_sums, sums, sizeof(s.h_sums), hipMemcpyDeviceToHost, s.stream));
    return TBK_OK;
}

// Q at n probes over all slabs: every slab's kernels are enqueued first, then every stream is waited for; the host adds the integers
int fermi_probe(std::vector<FermiSlab>& slabs, const double* energies, int n, FermiCount* q) {
    for (FermiSlab& s : slabs) TBK_CHECK(fermi_probe_enqueue(s, energies, n));
    for (int m = 0; m < n; ++m) q[m] = FermiCount();
    for (FermiSlab& s : slabs) {
        TBK_HIP(hipSetDevice(s.device));
        TBK_HIP(hipStreamSynchronize(s.stream));
        for (int m = 0; m < n; ++m) q[m].add(fermi_count(s.h_sums + 3 * m));
    }
    return TBK_OK;
}

// emin / emax [n_orb] over all slabs, through every slab's h_edges
int fermi_edges(std::vector<FermiSlab>& slabs, int n_orb, double* emin, double* emax) {
    for (FermiSlab& s : slabs) {
        TBK_HIP(hipSetDevice(s.device));
        auto* pmin = reinterpret_cast<double*>(s.d_ws + s.L.off_pmin);
        auto* pmax = reinterpret_cast<double*>(s.d_ws + s.L.off_pmax);
        auto* d_min = reinterpret_cast<double*>(s.d_ws + s.L.off_emin);
        auto* d_max = reinterpret_cast<double*>(s.d_ws + s.L.off_emax);
        const dim3 grid((unsigned)s.L.edge_wg, (unsigned)((n_orb + FERMI_THREADS - 1) / FERMI_THREADS));
        if (s.ev) s.ev->start();
        hipLaunchKernelGGL(band_edges_kernel, grid, dim3(FERMI_THREADS), 0, s.stream, s.d_E, s.L.rows, n_orb, pmin, pmax);
        TBK_HIP(hipGetLastError());
        hipLaunchKernelGGL(band_edges_reduce_kernel, dim3(grid.y), dim3(FERMI_THREADS), 0, s.stream, pmin, pmax, s.L.edge_wg, n_orb, d_min, d_max);
        TBK_HIP(hipGetLastError());
        if (s.ev) s.ev->stop();
        double* h = s.h_edges.data();
        TBK_HIP(hipMemcpyAsync(h, d_min, (size_t)n_orb * sizeof(double), hipMemcpyDeviceToHost, s.stream));
        TBK_HIP(hipMemcpyAsync(h + n_orb, d_max, (size_t)n_orb * sizeof(double), hipMemcpyDeviceToHost, s.stream));
    }
    for (size_t i = 0; i < slabs.size(); ++i) {
        FermiSlab& s = slabs[i];
        TBK_HIP(hipSetDevice(s.device));
        TBK_HIP(hipStreamSynchronize(s.stream));
        const double* h = s.h_edges.data();
        for (int b = 0; b < n_orb; ++b) {
            emin[b] = i == 0 ? h[b] : std::fmin(emin[b], h[b]);
            emax[b] = i == 0 ? h[n_orb + b] : std::fmax(emax[b], h[n_orb + b]);
        }
    }
    return TBK_OK;
}

// ---- the search on doubles -------------------------------------------------------------------------------------------------------
// the ordered-integer image of the doubles: x < y  <=>  key(x) < key(y) (-0.0 is the double in front of +0.0)
unsigned long long fermi_key(double x) {
    unsigned long long b;
    std::memcpy(&b, &x, sizeof(b));
    return (b >> 63) ? ~b : b | (1ull << 63);
}
double fermi_unkey(unsigned long long k) {
    const unsigned long long b = (k >> 63) ? k & ~(1ull << 63) : ~k;
    double x;
    std::memcpy(&x, &b, sizeof(x));
    return x;
}

// mu, lower, upper, N(mu) for n_electrons in (0, n_orb) (include/tbk.h); simplices = S * NK of the whole mesh
int fermi_search(std::vector<FermiSlab>& slabs, int n_orb, int64_t simplices, double n_electrons, double* out, int* passes_out) {
    std::vector<double> emin((size_t)n_orb), emax((size_t)n_orb);
    TBK_CHECK(fermi_edges(slabs, n_orb, emin.data(), emax.data()));
    *passes_out = 0;
    // the gap case: the doubles of the eigenvalue array, no search (fixed point cannot see the band edge: DESIGN 12.3)
    if (n_electrons == std::floor(n_electrons)) {
        const int m = (int)n_electrons;  // 1 .. n_orb - 1
        if (emax[(size_t)m - 1] < emin[(size_t)m]) {
            const double lower = emax[(size_t)m - 1], upper = emin[(size_t)m];
            out[0] = lower + (upper - lower) / 2;
            out[1] = lower;
            out[2] = upper;
            out[3] = (double)m;  // every simplex of the bands below is full, none of those above has begun: the kernel's N, exactly
            return TBK_OK;
        }
    }
    const FermiCount target = fermi_target(n_electrons, simplices);
    double lo = std::nextafter(emin[0], -INFINITY), hi = emax[(size_t)n_orb - 1];  // Q(lo) = 0 < t <= Q(hi) = n_orb S NK 2^40
    TBK_ARG(std::isfinite(lo) && std::isfinite(hi) && lo < hi, "the eigenvalues are not finite");
    FermiCount q_hi;
    q_hi.whole = (unsigned long long)n_orb * (unsigned long long)simplices;
    double probes[FERMI_PROBES];
    FermiCount q[FERMI_PROBES];
    bool first = true;
    while (fermi_key(hi) - fermi_key(lo) > 1) {
        int n = 0;
        if (first && lo < 0.0 && hi > 0.0) {
            // A bracket around zero: the image of the negative doubles runs against that of the positive ones, so equidistant
            // points in it would not follow a scaling of the energies.  One pass of points that do: 0 and lo, hi times 2^-256 j.
            // Every sub-interval is then at most 256 binades = 2^60 doubles long (points that underflow to zero are left out; the
            // interval next to zero then ends below 2^-818 and is shorter still): 15 more passes.
            for (int j = 1; j <= 7; ++j) {
                const double x = std::ldexp(lo, -256 * j);
                if (x < 0.0 && x > lo) probes[n++] = x;
            }
            probes[n++] = 0.0;
            for (int j = 7; j >= 1; --j) {
                const double x = std::ldexp(hi, -256 * j);
                if (x > 0.0 && x < hi) probes[n++] = x;
            }
        } else {
            const unsigned long long k_lo = fermi_key(lo), gap = fermi_key(hi) - k_lo;
            n = (int)std::min<unsigned long long>(FERMI_SEARCH_M, gap - 1);
            for (int j = 1; j <= n; ++j)
                probes[j - 1] = fermi_unkey(k_lo + (unsigned long long)(((unsigned __int128)gap * (unsigned)j) / (unsigned)(n + 1)));
        }
        first = false;
        TBK_CHECK(fermi_probe(slabs, probes, n, q));
        *passes_out += 1;
        int j = 0;
        while (j < n && !q[j].at_least(target)) ++j;  // the first probe with Q >= t
        if (j > 0) lo = probes[j - 1];
        if (j < n) {
            hi = probes[j];
            q_hi = q[j];
        }
        if (lo == 0.0 && hi > 0.0) lo = 0.0;                      // +0.0: the double in front of the positive ones
        if (hi == 0.0 && lo < 0.0) hi = -0.0;                     // -0.0: the double behind the negative ones
        TBK_ARG(*passes_out <= 64, "the Fermi-level search does not end (N(E) is not a number?)");
    }
    const double mu = hi == 0.0 ? 0.0 : hi;
    out[0] = out[1] = out[2] = mu;
    out[3] = fermi_nos(q_hi, simplices);
    return TBK_OK;
}

int fermi_check_electrons(double n_electrons, int n_orb) {
    TBK_ARG(std::isfinite(n_electrons) && n_electrons > 0.0 && n_electrons < (double)n_orb, "n_electrons must lie inside (0, n_orb)");
    return TBK_OK;
}

// eigenvalues the caller brought, on the device just checked: one slab that is the whole mesh, on the null stream, not timed
struct FermiOwned {
    TetraOwnedE d_E;
    DevBuf d_ws;
    std::vector<FermiSlab> slabs;
    int make(int device, int dim, const int32_t* mesh, int n_orb, const double* E, int64_t nk) {
        slabs.resize(1);
        FermiSlab& s = slabs[0];
        s.device = device;
        s.dim = dim;
        s.h_edges.resize(2 * (size_t)n_orb);
        TBK_CHECK(fermi_plan(dim, mesh, mesh[0], mesh[0], n_orb, &s.L));
        TBK_CHECK(d_E.upload(E, nk, n_orb));
        TBK_CHECK(d_ws.reserve(s.L.ws_bytes));
        s.d_E = d_E.d();
        s.d_ws = d_ws.as<char>();
        return TBK_OK;
    }
};

// The Fermi state of a staged slab, on its handle's device: the plan and the probe rows in ws_dos -- in front of the slab's
// eigenvalues (TetraStaged::make) or, for a family that finds its mu on eigenvalues it keeps, behind them
int fermi_reserve(const TetraStaged& t, const TetraSlab& s, const int32_t* mesh, FermiSlab* f) {
    f->device = s.m->device;
    f->dim = t.dim;
    f->stream = s.m->stream;
    f->h_edges.resize(2 * (size_t)t.n_orb);
    TBK_CHECK(fermi_plan(t.dim, mesh, s.p_count, s.upper_planes(), t.n_orb, &f->L));
    return s.m->ws_dos.reserve(f->L.ws_bytes);
}

void fermi_attach(const TetraStaged& t, std::vector<FermiSlab>& state) {
    for (size_t i = 0; i < state.size(); ++i) {
        state[i].d_E = t.slabs[i].own_E(t.n_orb);
        state[i].d_ws = t.slabs[i].m->ws_dos.as<char>();
    }
}

int64_t fermi_simplices(const TetraStaged& t) { return (int64_t)(t.dim == 3 ? 6 : 2) * t.nk_total; }

// The mesh on staged handles: handle i takes the slab of tbk_dos_multi, and its eigenvalues stay in its ws_out across all passes.
// `state` is the caller's, declared in front of `staged`.  The kernels of every pass are booked on the handles' recorders.
int fermi_make(TetraStaged& staged, std::vector<FermiSlab>& state, tbk_model* const* handles, int n_handles, const int32_t* mesh) {
    TBK_CHECK(staged.make(handles, n_handles, mesh, DOS_MESH, false, [&](TetraSlab& s, size_t i) {
        state.resize(i + 1);  // (nothing is enqueued into the state before the first pass)
        state[i].ev = s.ev;
        return fermi_reserve(staged, s, mesh, &state[i]);
    }));
    fermi_attach(staged, state);
    return TBK_OK;
}

// every call counts, and the passes of a search
int fermi_book(TetraStaged& staged, int passes) {
    TBK_CHECK(staged.streams.book(TIMED_FERMI));
    for (TetraSlab& s : staged.slabs) s.m->timed[TIMED_FERMI].passes += passes;
    return TBK_OK;
}

}  // namespace

int tbk_fermi_check_electrons(double n_electrons, int n_orb) { return fermi_check_electrons(n_electrons, n_orb); }

int tbk_fermi_resident(TetraStaged& staged, std::vector<FermiSlab>& state, const int32_t* mesh, int mode, double value, double* out4) {
    state.resize(staged.slabs.size());
    for (size_t i = 0; i < state.size(); ++i) {
        TBK_HIP(hipSetDevice(staged.slabs[i].m->device));
        TBK_CHECK(fermi_reserve(staged, staged.slabs[i], mesh, &state[i]));
    }
    fermi_attach(staged, state);
    if (mode == 1) {
        int passes = 0;
        return fermi_search(state, staged.n_orb, fermi_simplices(staged), value, out4, &passes);
    }
    FermiCount q[FERMI_PROBES];
    TBK_CHECK(fermi_probe(state, &value, 1, q));
    out4[0] = out4[1] = out4[2] = value;
    out4[3] = fermi_nos(q[0], fermi_simplices(staged));
    return TBK_OK;
}

extern "C" int tbk_nos_at_from_eigenvalues(int device, int dim, const int32_t* mesh, int n_orb, const double* E, const double* energies,
                                           int64_t n_p, double* nos_out) {
    int64_t nk = 0;
    TBK_CHECK(tetra_check_mesh(dim, mesh, DOS_MESH, &nk));
    TBK_ARG(E != nullptr && energies != nullptr && nos_out != nullptr, "E / energies / nos is NULL");
    TBK_ARG(n_orb >= 1, "n_orb < 1");
    TBK_ARG(n_p >= 1, "no probe energies");
    for (int64_t j = 0; j < n_p; ++j) TBK_ARG(std::isfinite(energies[j]), "a probe energy is not finite");
    TBK_CHECK(tetra_check_device(device));
    FermiOwned own;
    TBK_CHECK(own.make(device, dim, mesh, n_orb, E, nk));
    const int64_t simplices = (int64_t)(dim == 3 ? 6 : 2) * nk;
    FermiCount q[FERMI_PROBES];
    for (int64_t j0 = 0; j0 < n_p; j0 += FERMI_PROBES) {
        const int n = (int)std::min<int64_t>(FERMI_PROBES, n_p - j0);
        TBK_CHECK(fermi_probe(own.slabs, energies + j0, n, q));
        for (int m = 0; m < n; ++m) nos_out[j0 + m] = fermi_nos(q[m], simplices);
    }
    return TBK_OK;
}

extern "C" int tbk_band_edges_from_eigenvalues(int device, int dim, const int32_t* mesh, int n_orb, const double* E, double* emin_out,
                                               double* emax_out) {
    int64_t nk = 0;
    TBK_CHECK(tetra_check_mesh(dim, mesh, DOS_MESH, &nk));
    TBK_ARG(E != nullptr && emin_out != nullptr && emax_out != nullptr, "E / emin / emax is NULL");
    TBK_ARG(n_orb >= 1, "n_orb < 1");
    TBK_CHECK(tetra_check_device(device));
    FermiOwned own;
    TBK_CHECK(own.make(device, dim, mesh, n_orb, E, nk));
    return fermi_edges(own.slabs, n_orb, emin_out, emax_out);
}

extern "C" int tbk_fermi_from_eigenvalues(int device, int dim, const int32_t* mesh, int n_orb, const double* E, double n_electrons, double* out,
                                          int32_t* passes_out) {
    int64_t nk = 0;
    TBK_CHECK(tetra_check_mesh(dim, mesh, DOS_MESH, &nk));
    TBK_ARG(E != nullptr && out != nullptr, "E / out is NULL");
    TBK_ARG(n_orb >= 1, "n_orb < 1");
    TBK_CHECK(fermi_check_electrons(n_electrons, n_orb));
    TBK_CHECK(tetra_check_device(device));
    FermiOwned own;
    TBK_CHECK(own.make(device, dim, mesh, n_orb, E, nk));
    int passes = 0;
    TBK_CHECK(fermi_search(own.slabs, n_orb, (int64_t)(dim == 3 ? 6 : 2) * nk, n_electrons, out, &passes));
    if (passes_out) *passes_out = passes;
    return TBK_OK;
}

extern "C" int tbk_band_edges_multi(tbk_model* const* handles, int n_handles, const int32_t* mesh, double* emin_out, double* emax_out) {
    TBK_ARG(emin_out != nullptr && emax_out != nullptr, "emin / emax is NULL");
    std::vector<FermiSlab> state;  // (in front of `staged`: its streams wait before the state goes)
    TetraStaged staged;
    TBK_CHECK(fermi_make(staged, state, handles, n_handles, mesh));
    TBK_CHECK(fermi_edges(state, staged.n_orb, emin_out, emax_out));
    return fermi_book(staged, 0);
}

extern "C" int tbk_band_edges(tbk_model* m, const int32_t* mesh, double* emin_out, double* emax_out) {
    return tbk_band_edges_multi(&m, 1, mesh, emin_out, emax_out);
}

extern "C" int tbk_fermi_multi(tbk_model* const* handles, int n_handles, const int32_t* mesh, double n_electrons, double* out) {
    TBK_ARG(out != nullptr, "out is NULL");
    TBK_ARG(handles != nullptr && n_handles >= 1 && handles[0] != nullptr, "no handles");
    TBK_CHECK(fermi_check_electrons(n_electrons, handles[0]->n_orb));
    std::vector<FermiSlab> state;  // (in front of `staged`: its streams wait before the state goes)
    TetraStaged staged;
    TBK_CHECK(fermi_make(staged, state, handles, n_handles, mesh));
    int passes = 0;
    TBK_CHECK(fermi_search(state, staged.n_orb, fermi_simplices(staged), n_electrons, out, &passes));
    return fermi_book(staged, passes);
}

extern "C" int tbk_fermi(tbk_model* m, const int32_t* mesh, double n_electrons, double* out) { return tbk_fermi_multi(&m, 1, mesh, n_electrons, out); }

extern "C" int tbk_fermi_timing(tbk_model* m, double* ms, int64_t* calls, int64_t* passes, int reset) {
    TBK_ARG(m != nullptr && ms != nullptr && calls != nullptr && passes != nullptr, "model / ms / calls / passes is NULL");
    return tbk_timed_read(m, TIMED_FERMI, 1, ms, calls, passes, reset);
}
