// tbk_berry.hip -- the lattice Berry flux (Fukui-Hatsugai-Suzuki field strength) and the Chern numbers of a uniform, periodic k mesh.
// Not in the reference; DESIGN.md section 18 has the quantity, the kernels, the error bound and the measurements, tools/berry_model.py
// is the statement the tests compare with.
//
//   M_d(k)     = U[k][:, lo:hi]^H D(e_d) U[k+e_d][:, lo:hi]           U of tbk_eigh_device (convention 2), D: 1 or the orbital phases
//   L_d(k)     = det M_d(k)                                            of convention 1 for q = e_d (a host table); [lo, hi): a band set
//   a_d(k)     = round(arg L_d(k) / (2 pi) 2^64) mod 2^64              the uint64 angle word, 0 for L = 0
//   F_ab(k)    = a_a(k) + a_b(k+e_a) - a_a(k+e_b) - a_b(k)             wrapping 64-bit arithmetic, read as int64
//   flux_ab(k) = (double)F_ab(k) 2 pi 2^-64,   C_ab(i_c) = (sum of F_ab over the plane) / 2^64, an integer
//
//   berry_link_kernel<BT, false>  M as four real products on v_mfma_f64_16x16x4_f64 by zpanel_overlap (tbk_zmfma.h): panels of 16
//                       orbitals through LDS, orbital-major planes Ur, Ui (bands of the set at k) and Re, Im of D U' (at k+e_d),
//                       padded with zeros to the tile; a panel row of the set is the contiguous segment U[k][i][lo:hi], D is applied
//                       while staging.  M is never stored to global memory: the accumulators go to an LDS tile (over the planes,
//                       which are done with) and the tile is factored there: per column one pivot search (every wave by itself, lane =
//                       row, largest |Re| + |Im|, a tie to the lowest row), two barriers, one rank-1 update with a thread per column
//                       and row group -- the swap is implicit: the row that gives the pivot is read before the barrier and takes the
//                       updated former row j behind it.  The determinant is the product of the pivots in column order with the
//                       parity of the swaps.  BT = 1: m <= 16, a link per wave and four per workgroup, a 16 x 16 tile each;
//                       BT = 4: m <= 64, a link per workgroup, a 64 x 64 tile (65 KiB with its padding), the updates over all 256
//                       threads.  Per link: L (complex), the angle word and |L|.
//   berry_link_kernel<4, true>    m > 64: the same product, a workgroup per 64 x 64 block of M, written to a batch workspace;
//                       rocsolver_zgetrf_strided_batched factors the batch (the split tbk_eigh makes, calls below 2^29 elements) and
//   berry_det_kernel    multiplies the diagonal in index order and applies the pivot parity.
//   berry_flux_kernel   the integer plaquette arithmetic: a workgroup per (set, plane, i_c) walks its plane, one owner per
//                       (set, plane, k) writes the flux, the plane sum goes as two 64-bit sums of the 32-bit halves through a fixed
//                       tree to the (high, low) words of the 128-bit total: the high word is the Chern number, the low one is 0.  One
//                       more workgroup per set takes the minimum of |L|.  No atomics.
//
// Every set has its own launches, so the bits of a link depend on U(k), U(k+e_d), D, lo and hi alone: not on the other sets, the
// batch, the share of the mesh a handle takes or the handle.

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include <rocsolver/rocsolver.h>

#include "tbk_occ.h"  // OCC_MESH
#include "tbk_resident.h"
#include "tbk_zmfma.h"

namespace {

constexpr int BERRY_THREADS = 256;
constexpr int BERRY_MAX_SETS = 16;
constexpr int BERRY_MAX_ORB = 16320;                        // 255 x 255 blocks of one M: one grid row each
constexpr int64_t BERRY_MAX_LAUNCH = int64_t(1) << 30;      // links per launch (grid x), at most
constexpr int64_t BERRY_LIB_ELEMENTS = int64_t(1) << 29;    // rocSOLVER calls stay below this many elements (tbk_eigh.hip)
constexpr size_t BERRY_WS_BUDGET = size_t(256) << 20;       // M of one batch of the library path, at most
constexpr double BERRY_TWO_PI = 6.283185307179586476925286766559;

struct BerryMesh {
    int n[3];    // (n[2] = 1 in two dimensions)
    int dim;
    int64_t nk;  // points of the mesh
};

// one band set: where it starts, its size, the template (1, 4, or 64: the library path) and the links per launch
struct BerrySet {
    int lo = 0, m = 0, bt = 0;
    int64_t batch = 1;
};

// the one place that chooses
BerrySet berry_plan_set(int64_t nk, int lo, int hi) {
    BerrySet s;
    s.lo = lo;
    s.m = hi - lo;
    s.bt = s.m <= 16 ? 1 : s.m <= 64 ? 4 : 64;
    const int64_t links = 3 * nk;
    if (s.bt == 64) {
        const int64_t m2 = (int64_t)s.m * s.m;
        s.batch = std::max<int64_t>(1, std::min(BERRY_LIB_ELEMENTS / m2, (int64_t)(BERRY_WS_BUDGET / (sizeof(double2) * (size_t)m2))));
    } else {
        s.batch = BERRY_MAX_LAUNCH;
    }
    s.batch = std::min(s.batch, links);
    return s;
}

// LDS of one workgroup of berry_link_kernel: the planes, and over them the tile(s)
constexpr int berry_plane_stride(int bt) { return bt == 1 ? ZPanel<1>::S : ZPanel<4>::S; }
constexpr int berry_tile_stride(int bt) { return 16 * bt + 1; }
constexpr size_t berry_lds_bytes(int bt, bool store) {
    const size_t kpw = bt == 1 ? 4 : 1;
    const size_t planes = kpw * 4 * 16 * (size_t)berry_plane_stride(bt) * sizeof(double);
    const size_t tiles = store ? 0 : kpw * (size_t)(16 * bt) * (size_t)berry_tile_stride(bt) * sizeof(double2);
    return planes > tiles ? planes : tiles;
}

// the length of axis d and the distance of its neighbours in the flat index (selects, not indexed loads: d is a run-time value)
__device__ __forceinline__ int64_t berry_length(const BerryMesh& g, int d) { return d == 0 ? g.n[0] : d == 1 ? g.n[1] : g.n[2]; }
__device__ __forceinline__ int64_t berry_stride(const BerryMesh& g, int d) {
    return d == 0 ? (int64_t)g.n[1] * g.n[2] : d == 1 ? (int64_t)g.n[2] : 1;
}

// the flat index of k+e_d
__device__ __forceinline__ int64_t berry_next(const BerryMesh& g, int64_t k, int d) {
    const int64_t stride = berry_stride(g, d), len = berry_length(g, d);
    const int64_t idx = (k / stride) % len;
    return idx + 1 == len ? k - idx * stride : k + stride;
}

__device__ __forceinline__ double2 berry_cmul(double2 a, double2 b) {
    return make_double2(fma(a.x, b.x, -(a.y * b.y)), fma(a.x, b.y, a.y * b.x));
}

// 1 / z without an overflow of |z|^2 (0 for z = 0: a dead column updates nothing)
__device__ __forceinline__ double2 berry_reciprocal(double2 z) {
    const double s = fabs(z.x) + fabs(z.y);
    if (!(s > 0.0)) return make_double2(0.0, 0.0);
    const double a = z.x / s, b = z.y / s;
    const double d = (a * a + b * b) * s;
    return make_double2(a / d, -b / d);
}

// round(arg L / (2 pi) 2^64) mod 2^64; 0 for L = 0
__device__ __forceinline__ uint64_t berry_word(double2 L) {
    if (L.x == 0.0 && L.y == 0.0) return 0;
    const double turns = atan2(L.y, L.x) / BERRY_TWO_PI;  // in [-1/2, 1/2]
    const double x = rint(ldexp(turns, 64));              // a whole number in [-2^63, 2^63]
    const double mag = fabs(x);
    const uint64_t u = mag >= 9223372036854775808.0 ? uint64_t(1) << 63 : (uint64_t)mag;
    return x < 0.0 ? uint64_t(0) - u : u;
}

// BT tiles of 16 along each side of the workgroup's block of M: 4 (one link per workgroup, wave t owns tile row t) or 1 (m <= 16: four
// links per workgroup, one per wave).  The links of this launch are l0 .. l0 + gridDim.x KPW of the n_links = dim nkc links of the
// mesh points [k0, k0 + nkc): link l is axis l / nkc at point k0 + l % nkc, and the outputs of the set are [dim][nkc] = [n_links].
// D: NULL or [dim][n] complex.  STORE (BT = 4): blockIdx.y is the 64 x 64 block of M, written to Mws[l - l0][m][m]; else M stays in
// LDS and L, the word and |L| of the link are written.  Dynamic LDS: berry_lds_bytes(BT, STORE).
template <int BT, bool STORE>
__global__ void __launch_bounds__(BERRY_THREADS) berry_link_kernel(const double2* __restrict__ U, BerryMesh g, int n, int lo, int m,
                                                                   const double2* __restrict__ D, int64_t k0, int64_t nkc, int64_t l0,
                                                                   int64_t n_links, double2* __restrict__ Mws, double2* __restrict__ L_out,
                                                                   uint64_t* __restrict__ words, double* __restrict__ absL) {
    using Geo = ZPanel<BT>;  // (tbk_zmfma.h; an item is a link)
    constexpr int RB = Geo::RB, KPW = Geo::KPW, TEAM = Geo::TEAM;
    static_assert(BERRY_THREADS == Geo::THREADS, "the panel's workgroup");
    constexpr int TS = berry_tile_stride(BT); // complex numbers between the rows of the tile: a wave walks along a row
    extern __shared__ double2 berry_lds[];
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int team = BT == 1 ? wave : 0, tt = tid - team * TEAM;
    const int nb = (m + RB - 1) / RB;
    const int bi = STORE ? (int)blockIdx.y / nb : 0, bj = STORE ? (int)blockIdx.y - bi * nb : 0;
    const int64_t li = l0 + (int64_t)blockIdx.x * KPW + team;
    const bool valid = li < n_links;
    const int d = valid ? (int)(li / nkc) : 0;
    const int64_t k = valid ? k0 + (li - (int64_t)d * nkc) : 0;
    const int64_t kp = berry_next(g, k, d);
    const double2* Uk = U + (size_t)k * n * n + lo;
    const double2* Up = U + (size_t)kp * n * n + lo;
    const double2* Dd = D ? D + (size_t)d * n : nullptr;
    double* pl = reinterpret_cast<double*>(berry_lds) + (size_t)team * 4 * 16 * Geo::S;  // the team's four planes
    const int ti = BT == 1 ? 0 : wave;                      // the wave's tile row
    const bool row_live = valid && bi * RB + ti * 16 < m;   // (wave-uniform)
    zd4 accr[BT], acci[BT];
    zpanel_overlap<BT>(Uk, Up, Dd, valid, n, m, bi, bj, pl, tt, ti, lane, row_live, accr, acci);  // M = U(k)^H D U(k+e_d) of the set
    // lane (q, c), register r: row q + 4 r, column c of the tile
    if constexpr (STORE) {
        if (!row_live) return;
        ztiles_store<BT>(Mws + (size_t)(li - l0) * m * m, m, bi * RB + ti * 16, bj * RB, lane, accr, acci);
        return;
    } else {
        double2* T = berry_lds + (size_t)team * RB * TS;
        __syncthreads();  // the last panel has been read: the tile lies over the planes
        if (row_live) {
#pragma unroll
            for (int tj = 0; tj < BT; ++tj) {
                if (tj * 16 < m) {  // (uniform)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        T[(ti * 16 + (lane >> 4) + 4 * r) * TS + tj * 16 + (lane & 15)] = make_double2(accr[tj][r], acci[tj][r]);
                }
            }
        }
        // LU with partial pivoting in the tile; every thread of the team carries the determinant.  m is the launch's: all teams
        // of the workgroup keep the same barriers, a team without a link factors what its tile holds and writes nothing.
        const int c = tt % RB, g4 = tt / RB;  // this thread's column and its rows g4 + 4 r
        const int prow = lane % RB;           // the row this lane looks at in the pivot search
        double2 det = make_double2(1.0, 0.0);
        bool dead = false;
        for (int j = 0; j < m; ++j) {
            __syncthreads();  // the tile, or the update of column j - 1, is written
            double best = -1.0;
            int p = prow;
            if (valid && prow >= j && prow < m) {
                const double2 v = T[prow * TS + j];
                best = fabs(v.x) + fabs(v.y);
            }
#pragma unroll
            for (int off = RB / 2; off >= 1; off >>= 1) {
                const double ob = __shfl_xor(best, off, 64);
                const int oi = __shfl_xor(p, off, 64);
                if (ob > best || (ob == best && oi < p)) {
                    best = ob;
                    p = oi;
                }
            }
            if (!valid) p = j;
            const bool col_on = valid && c > j && c < m;
            const double2 piv = valid ? T[p * TS + j] : make_double2(1.0, 0.0);
            const double2 tjj = valid ? T[j * TS + j] : piv;
            double2 prc = make_double2(0.0, 0.0), jrc = prc;
            if (col_on) {
                prc = T[p * TS + c];
                jrc = T[j * TS + c];
            }
            __syncthreads();  // everyone has read the pivot row: row p may take the updated former row j
            if (piv.x == 0.0 && piv.y == 0.0) dead = true;
            det = berry_cmul(det, piv);
            if (p != j) det = make_double2(-det.x, -det.y);
            const double2 inv = berry_reciprocal(piv);
            if (col_on) {
#pragma unroll
                for (int r = 0; r < RB / 4; ++r) {
                    const int i = g4 + 4 * r;
                    if (i > j && i < m) {
                        const double2 lij = i == p ? tjj : T[i * TS + j];
                        const double2 base = i == p ? jrc : T[i * TS + c];
                        const double2 f = berry_cmul(lij, inv);
                        const double2 fp = berry_cmul(f, prc);
                        T[i * TS + c] = make_double2(base.x - fp.x, base.y - fp.y);
                    }
                }
            }
        }
        if (valid && tt == 0) {
            if (dead) det = make_double2(0.0, 0.0);
            L_out[li] = det;
            words[li] = berry_word(det);
            absL[li] = hypot(det.x, det.y);
        }
    }
}

// the library path's last step: L = parity * product of the diagonal of the factored M in index order.  One thread per link of the batch
__global__ void __launch_bounds__(BERRY_THREADS) berry_det_kernel(const double2* __restrict__ A, const int* __restrict__ ipiv, int m, int64_t count,
                                                                  double2* __restrict__ L_out, uint64_t* __restrict__ words,
                                                                  double* __restrict__ absL) {
    const int64_t b = (int64_t)blockIdx.x * BERRY_THREADS + threadIdx.x;
    if (b >= count) return;
    const double2* a = A + (size_t)b * m * m;
    const int* piv = ipiv + (size_t)b * m;
    double2 det = make_double2(1.0, 0.0);
    bool dead = false;
    for (int i = 0; i < m; ++i) {
        const double2 v = a[(size_t)i * m + i];
        if (v.x == 0.0 && v.y == 0.0) dead = true;
        det = berry_cmul(det, v);
        if (piv[i] != i + 1) det = make_double2(-det.x, -det.y);
    }
    if (dead) det = make_double2(0.0, 0.0);
    L_out[b] = det;
    words[b] = berry_word(det);
    absL[b] = hypot(det.x, det.y);
}

// grid (slices + 1, sets).  blockIdx.x < slices: the plane (a, b) at index i_c of the remaining axis (two dimensions: the one plane);
// flux[s][p][k] for its points, chern[s][slice] and low[s][slice] the high and low words of the 128-bit sum of F.  blockIdx.x == slices:
// link_min[s] = the minimum of absL[s][.][.] (absL NULL: nothing).  words: [sets][dim][NK]
__global__ void __launch_bounds__(BERRY_THREADS) berry_flux_kernel(const uint64_t* __restrict__ words, const double* __restrict__ absL, BerryMesh g,
                                                                   int slices, double* __restrict__ flux, int64_t* __restrict__ chern,
                                                                   uint64_t* __restrict__ low, double* __restrict__ link_min) {
    __shared__ int64_t red_hi[BERRY_THREADS], red_lo[BERRY_THREADS];
    __shared__ double red_min[BERRY_THREADS];
    const int tid = (int)threadIdx.x;
    const int s = (int)blockIdx.y;
    const int x = (int)blockIdx.x;
    if (x == slices) {
        if (absL == nullptr) return;
        const double* v = absL + (size_t)s * g.dim * g.nk;
        const int64_t count = (int64_t)g.dim * g.nk;
        double least = INFINITY;
        for (int64_t i = tid; i < count; i += BERRY_THREADS) least = fmin(least, v[i]);
        red_min[tid] = least;
        __syncthreads();
        for (int w = BERRY_THREADS / 2; w >= 1; w >>= 1) {
            if (tid < w) red_min[tid] = fmin(red_min[tid], red_min[tid + w]);
            __syncthreads();
        }
        if (tid == 0) link_min[s] = red_min[0];
        return;
    }
    int p = 0, a = 0, b = 1, c = 2, ic = x;
    if (g.dim == 3) {
        if (x >= g.n[2] + g.n[1]) {
            p = 2, a = 1, b = 2, c = 0, ic = x - g.n[2] - g.n[1];
        } else if (x >= g.n[2]) {
            p = 1, a = 0, b = 2, c = 1, ic = x - g.n[2];
        }
    } else {
        ic = 0;  // (n[2] = 1: the third index of every point)
    }
    const int planes = g.dim == 3 ? 3 : 1;
    const uint64_t* wa = words + ((size_t)s * g.dim + a) * g.nk;
    const uint64_t* wb = words + ((size_t)s * g.dim + b) * g.nk;
    double* out = flux + ((size_t)s * planes + p) * g.nk;
    const int64_t len_b = berry_length(g, b), count = berry_length(g, a) * len_b;
    const int64_t step_a = berry_stride(g, a), step_b = berry_stride(g, b), base = ic * berry_stride(g, c);
    const double turn = ldexp(BERRY_TWO_PI, -64);
    int64_t hi = 0, lo = 0;
    for (int64_t t = tid; t < count; t += BERRY_THREADS) {
        const int64_t k = (t / len_b) * step_a + (t % len_b) * step_b + base;
        const int64_t ka = berry_next(g, k, a), kb = berry_next(g, k, b);
        const int64_t F = (int64_t)(wa[k] + wb[ka] - wa[kb] - wb[k]);
        out[k] = (double)F * turn;
        hi += F >> 32;
        lo += F & 0xFFFFFFFFll;
    }
    red_hi[tid] = hi;
    red_lo[tid] = lo;
    __syncthreads();
    for (int w = BERRY_THREADS / 2; w >= 1; w >>= 1) {
        if (tid < w) {
            red_hi[tid] += red_hi[tid + w];
            red_lo[tid] += red_lo[tid + w];
        }
        __syncthreads();
    }
    if (tid == 0) {
        // total = hi 2^32 + lo with |hi| < 2^62 and 0 <= lo < 2^63: its low word, and the high one with the carry
        const uint64_t low_word = ((uint64_t)red_hi[0] << 32) + (uint64_t)red_lo[0];
        const int64_t carry = low_word < (uint64_t)red_lo[0] ? 1 : 0;
        chern[(size_t)s * slices + x] = (red_hi[0] >> 32) + carry;
        low[(size_t)s * slices + x] = low_word;
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
BerryMesh berry_mesh(int dim, const int32_t* mesh, int64_t nk) {
    BerryMesh g;
    g.n[0] = mesh[0];
    g.n[1] = mesh[1];
    g.n[2] = dim == 3 ? mesh[2] : 1;
    g.dim = dim;
    g.nk = nk;
    return g;
}

int berry_slices(int dim, const int32_t* mesh) { return dim == 3 ? mesh[0] + mesh[1] + mesh[2] : 1; }

int berry_check_sets(int n_orb, int n_sets, const int32_t* ranges, std::vector<BerrySet>* sets, int64_t nk) {
    TBK_ARG(n_sets >= 1 && n_sets <= BERRY_MAX_SETS, "n_sets must be 1 to 16");
    TBK_ARG(ranges != nullptr, "ranges is NULL");
    TBK_ARG(n_orb >= 1 && n_orb <= BERRY_MAX_ORB, "n_orb < 1 or more than 16320 orbitals");
    for (int s = 0; s < n_sets; ++s) {
        const int lo = ranges[2 * s], hi = ranges[2 * s + 1];
        TBK_ARG(lo >= 0 && hi <= n_orb && lo < hi, "a band set needs 0 <= lo < hi <= n_orb");
        if (sets) sets->push_back(berry_plan_set(nk, lo, hi));
    }
    return TBK_OK;
}

// the device memory the library path of these sets takes for one batch: M, the pivots, the flags (0: no set takes it)
size_t berry_lib_bytes(const std::vector<BerrySet>& sets, int64_t n_links) {
    size_t most = 0;
    for (const BerrySet& s : sets)
        if (s.bt == 64) {
            const size_t b = (size_t)std::min(s.batch, n_links);
            most = std::max(most, dos_align256(b * s.m * s.m * sizeof(double2)) + dos_align256(b * s.m * sizeof(int)) + dos_align256(b * sizeof(int)));
        }
    return most;
}

tbk_flag_row berry_raised;

// the links of every set at the mesh points [k0, k0 + nkc): d_L, d_words, d_abs are [sets][dim][nkc].  d_lib: berry_lib_bytes (the
// library path), blas: a handle on stream s (NULL when no set takes that path).  Stages of ev: 0 the link kernels, 1 the library's LU
int berry_launch_links(hipStream_t s, rocblas_handle blas, SpanRecorder* ev, const BerryMesh& g, int n, const std::vector<BerrySet>& sets,
                       const double* d_U, const double* d_D, int64_t k0, int64_t nkc, char* d_lib, double* d_L, uint64_t* d_words, double* d_abs) {
    const int64_t n_links = (int64_t)g.dim * nkc;
    const double2* U = reinterpret_cast<const double2*>(d_U);
    const double2* D = reinterpret_cast<const double2*>(d_D);
    for (size_t si = 0; si < sets.size(); ++si) {
        const BerrySet& b = sets[si];
        double2* L = reinterpret_cast<double2*>(d_L) + si * (size_t)n_links;
        uint64_t* W = d_words + si * (size_t)n_links;
        double* A = d_abs + si * (size_t)n_links;
        const int64_t batch = std::min(b.batch, n_links);
        for (int64_t l0 = 0; l0 < n_links; l0 += batch) {
            const int64_t nl = std::min(batch, n_links - l0);
            if (b.bt == 1) {
                if (ev) ev->start(0);
                hipLaunchKernelGGL((berry_link_kernel<1, false>), dim3((unsigned)((nl + 3) / 4)), dim3(BERRY_THREADS), berry_lds_bytes(1, false), s, U,
                                   g, n, b.lo, b.m, D, k0, nkc, l0, n_links, nullptr, L, W, A);
                if (ev) ev->stop();
                TBK_HIP(hipGetLastError());
            } else if (b.bt == 4) {
                TBK_HIP(tbk_raise_lds_limit(reinterpret_cast<const void*>(&berry_link_kernel<4, false>), (int)berry_lds_bytes(4, false), berry_raised));
                if (ev) ev->start(0);
                hipLaunchKernelGGL((berry_link_kernel<4, false>), dim3((unsigned)nl), dim3(BERRY_THREADS), berry_lds_bytes(4, false), s, U, g, n,
                                   b.lo, b.m, D, k0, nkc, l0, n_links, nullptr, L, W, A);
                if (ev) ev->stop();
                TBK_HIP(hipGetLastError());
            } else {
                const size_t m2 = (size_t)b.m * b.m;
                double2* Mws = reinterpret_cast<double2*>(d_lib);
                int* ipiv = reinterpret_cast<int*>(d_lib + dos_align256((size_t)batch * m2 * sizeof(double2)));
                int* info = reinterpret_cast<int*>(reinterpret_cast<char*>(ipiv) + dos_align256((size_t)batch * b.m * sizeof(int)));
                const int nbm = (b.m + 63) / 64;
                if (ev) ev->start(0);
                hipLaunchKernelGGL((berry_link_kernel<4, true>), dim3((unsigned)nl, (unsigned)(nbm * nbm)), dim3(BERRY_THREADS),
                                   berry_lds_bytes(4, true), s, U, g, n, b.lo, b.m, D, k0, nkc, l0, n_links, Mws, nullptr, nullptr, nullptr);
                if (ev) ev->stop();
                TBK_HIP(hipGetLastError());
                if (ev) ev->start(1);
                // (det M = det M^T: the row-major blocks are the library's column-major M^T)
                TBK_ROCBLAS(rocsolver_zgetrf_strided_batched(blas, b.m, b.m, reinterpret_cast<rocblas_double_complex*>(Mws), b.m,
                                                             (rocblas_stride)m2, ipiv, (rocblas_stride)b.m, info, (rocblas_int)nl));
                hipLaunchKernelGGL(berry_det_kernel, dim3((unsigned)((nl + BERRY_THREADS - 1) / BERRY_THREADS)), dim3(BERRY_THREADS), 0, s, Mws, ipiv,
                                   b.m, nl, L + l0, W + l0, A + l0);
                if (ev) ev->stop();
                TBK_HIP(hipGetLastError());
            }
        }
    }
    return TBK_OK;
}

// the outputs of the plaquette kernel in one device block: flux [S][P][NK], chern [S][slices], low [S][slices], link_min [S]
struct BerryOut {
    size_t off_chern = 0, off_low = 0, off_min = 0, bytes = 0;
    BerryOut(int n_sets, int planes, int64_t nk, int slices) {
        off_chern = dos_align256((size_t)n_sets * planes * nk * sizeof(double));
        off_low = off_chern + dos_align256((size_t)n_sets * slices * sizeof(int64_t));
        off_min = off_low + dos_align256((size_t)n_sets * slices * sizeof(uint64_t));
        bytes = off_min + dos_align256((size_t)n_sets * sizeof(double));
    }
};

int berry_launch_flux(hipStream_t s, SpanRecorder* ev, const BerryMesh& g, int n_sets, int slices, const uint64_t* d_words, const double* d_abs,
                      const BerryOut& o, char* d_out) {
    if (ev) ev->start(2);
    hipLaunchKernelGGL(berry_flux_kernel, dim3((unsigned)(slices + 1), (unsigned)n_sets), dim3(BERRY_THREADS), 0, s, d_words, d_abs, g, slices,
                       reinterpret_cast<double*>(d_out), reinterpret_cast<int64_t*>(d_out + o.off_chern),
                       reinterpret_cast<uint64_t*>(d_out + o.off_low), reinterpret_cast<double*>(d_out + o.off_min));
    if (ev) ev->stop();
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

// the low words of the plane sums are zero by construction (every angle word enters a closed plane once with each sign)
int berry_check_low(const std::vector<uint64_t>& low) {
    for (uint64_t v : low)
        if (v != 0) {
            tbk_set_error("the plaquettes of a closed plane did not add up to a multiple of 2^64");
            return TBK_ERR_DEVICE;
        }
    return TBK_OK;
}

constexpr const char* BERRY_FAMILY = "the Berry flux";

}  // namespace

extern "C" int tbk_berry_plan(int64_t nk, int n_orb, int n_sets, const int32_t* ranges, int64_t* out) {
    TBK_ARG(nk >= 1 && out != nullptr, "nk < 1 or out is NULL");
    std::vector<BerrySet> sets;
    TBK_CHECK(berry_check_sets(n_orb, n_sets, ranges, &sets, nk));
    for (int s = 0; s < n_sets; ++s) {
        out[2 * s] = sets[(size_t)s].bt;
        out[2 * s + 1] = sets[(size_t)s].batch;
    }
    return TBK_OK;
}

extern "C" int tbk_berry_links_from_eigensystem(int device, int dim, const int32_t* mesh, int n_orb, const double* U, int n_sets,
                                                const int32_t* ranges, const double* phases, double* L_out, uint64_t* words_out) {
    int64_t nk = 0;
    TBK_CHECK(tetra_check_mesh(dim, mesh, OCC_MESH, &nk));
    TBK_ARG(U != nullptr && L_out != nullptr && words_out != nullptr, "U / L / words is NULL");
    std::vector<BerrySet> sets;
    TBK_CHECK(berry_check_sets(n_orb, n_sets, ranges, &sets, nk));
    TBK_CHECK(tetra_check_device(device));
    const BerryMesh g = berry_mesh(dim, mesh, nk);
    const int64_t n_links = (int64_t)dim * nk;
    const size_t items = (size_t)n_sets * n_links;
    const size_t u_bytes = (size_t)nk * n_orb * n_orb * sizeof(double2), d_bytes = (size_t)dim * n_orb * sizeof(double2);
    const size_t lib_bytes = berry_lib_bytes(sets, n_links);
    DevBuf d_U, d_D, d_lib, d_L, d_W, d_A;
    TBK_CHECK(mesh_reserve(d_U, u_bytes, BERRY_FAMILY, "the eigenvectors of the whole mesh"));
    if (phases) TBK_CHECK(d_D.reserve(d_bytes));
    if (lib_bytes) TBK_CHECK(d_lib.reserve(lib_bytes));
    TBK_CHECK(d_L.reserve(items * sizeof(double2)));
    TBK_CHECK(d_W.reserve(items * sizeof(uint64_t)));
    TBK_CHECK(d_A.reserve(items * sizeof(double)));
    Owned<rocblas_handle, rocblas_destroy_handle> blas;
    if (lib_bytes) TBK_ROCBLAS(rocblas_create_handle(blas.put()));
    TBK_HIP(hipMemcpy(d_U.ptr, U, u_bytes, hipMemcpyHostToDevice));
    if (phases) TBK_HIP(hipMemcpy(d_D.ptr, phases, d_bytes, hipMemcpyHostToDevice));
    TBK_CHECK(berry_launch_links(nullptr, blas, nullptr, g, n_orb, sets, d_U.as<double>(), phases ? d_D.as<double>() : nullptr, 0, nk,
                                 d_lib.as<char>(), d_L.as<double>(), d_W.as<uint64_t>(), d_A.as<double>()));
    TBK_HIP(hipDeviceSynchronize());
    TBK_HIP(hipMemcpy(L_out, d_L.ptr, items * sizeof(double2), hipMemcpyDeviceToHost));
    TBK_HIP(hipMemcpy(words_out, d_W.ptr, items * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return TBK_OK;
}

extern "C" int tbk_berry_flux_from_links(int device, int dim, const int32_t* mesh, int n_sets, const uint64_t* words, double* flux_out,
                                         int64_t* chern_out) {
    int64_t nk = 0;
    TBK_CHECK(tetra_check_mesh(dim, mesh, OCC_MESH, &nk));
    TBK_ARG(n_sets >= 1 && n_sets <= BERRY_MAX_SETS, "n_sets must be 1 to 16");
    TBK_ARG(words != nullptr && flux_out != nullptr && chern_out != nullptr, "words / flux / chern is NULL");
    TBK_CHECK(tetra_check_device(device));
    const BerryMesh g = berry_mesh(dim, mesh, nk);
    const int slices = berry_slices(dim, mesh), planes = dim == 3 ? 3 : 1;
    const BerryOut o(n_sets, planes, nk, slices);
    const size_t w_bytes = (size_t)n_sets * dim * nk * sizeof(uint64_t);
    DevBuf d_W, d_out;
    TBK_CHECK(d_W.reserve(w_bytes));
    TBK_CHECK(d_out.reserve(o.bytes));
    TBK_HIP(hipMemcpy(d_W.ptr, words, w_bytes, hipMemcpyHostToDevice));
    TBK_CHECK(berry_launch_flux(nullptr, nullptr, g, n_sets, slices, d_W.as<uint64_t>(), nullptr, o, d_out.as<char>()));
    TBK_HIP(hipDeviceSynchronize());
    std::vector<uint64_t> low((size_t)n_sets * slices);
    TBK_HIP(hipMemcpy(flux_out, d_out.ptr, (size_t)n_sets * planes * nk * sizeof(double), hipMemcpyDeviceToHost));
    TBK_HIP(hipMemcpy(chern_out, d_out.as<char>() + o.off_chern, low.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
    TBK_HIP(hipMemcpy(low.data(), d_out.as<char>() + o.off_low, low.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return berry_check_low(low);
}

extern "C" int tbk_berry_flux_multi(tbk_model* const* handles, int n_handles, const int32_t* mesh, int n_sets, const int32_t* ranges,
                                    int convention, const double* pos, double* flux_out, int64_t* chern_out, double* link_min_out) {
    TBK_ARG(flux_out != nullptr && chern_out != nullptr && link_min_out != nullptr, "flux / chern / link_min is NULL");
    TBK_ARG(n_sets >= 1 && n_sets <= BERRY_MAX_SETS, "n_sets must be 1 to 16");
    TBK_ARG(ranges != nullptr, "ranges is NULL");
    TBK_CHECK(tbk_eigh_check_arguments(0, convention, pos));
    TetraHandles th;
    TBK_CHECK(th.open(handles, n_handles, mesh, OCC_MESH));
    const int dim = th.dim, n_orb = th.n_orb;
    const int64_t nk = th.nk_total;
    std::vector<BerrySet> sets;
    TBK_CHECK(berry_check_sets(n_orb, n_sets, ranges, &sets, nk));
    const BerryMesh g = berry_mesh(dim, mesh, nk);
    const int slices = berry_slices(dim, mesh), planes = dim == 3 ? 3 : 1;
    const BerryOut o(n_sets, planes, nk, slices);
    // (the host buffers the enqueued copies read and write, in front of `res`: its streams wait before they go)
    std::vector<double> h_D, h_abs, piece_a;
    std::vector<uint64_t> h_words, piece_w, low;
    ResidentMesh res;
    TBK_CHECK(res.open(dim, mesh, n_orb, nk));
    if (convention == 1) {
        int64_t unit[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int d = 0; d < dim; ++d) unit[d * dim + d] = 1;
        TBK_CHECK(mesh_phase_table(dim, mesh, n_orb, dim, unit, pos, &h_D));
    }
    // every handle holds the whole mesh's eigensystem and takes a contiguous share of the mesh points' links
    const TetraSlabs share(nk, n_handles);
    const bool alone = share.busy() == 1;
    const size_t d_bytes = h_D.size() * sizeof(double);
    const size_t all_links = (size_t)n_sets * dim * nk;
    std::vector<uint64_t*> dev_words((size_t)share.busy());
    std::vector<double*> dev_abs((size_t)share.busy());
    for (int i = 0; i < share.busy(); ++i) {
        tbk_model* m = handles[i];
        const int64_t k_lo = share.lo(i), k_n = share.count(i);
        const int64_t n_links = (int64_t)dim * k_n;
        const size_t items = (size_t)n_sets * n_links;
        TBK_CHECK(res.stage(m, BERRY_FAMILY, (size_t)nk * n_orb * sizeof(double), "the eigenvalues of the whole mesh", true));
        // ws_mesh_io: this handle's links L, words, |L|, then the phases; ws_mesh_work: (handle 0) the plaquette kernel's outputs and,
        // with several handles, the words and |L| of the whole mesh; behind them the library path's batch
        const size_t off_w = dos_align256(items * sizeof(double2)), off_a = off_w + dos_align256(items * sizeof(uint64_t));
        const size_t off_d = off_a + dos_align256(items * sizeof(double));
        TBK_CHECK(m->ws_mesh_io.reserve(off_d + d_bytes + 256));
        const size_t off_all = i == 0 ? dos_align256(o.bytes) : 0;
        const size_t off_lib = off_all + (i == 0 && !alone ? dos_align256(all_links * sizeof(uint64_t)) + dos_align256(all_links * sizeof(double)) : 0);
        const size_t lib_bytes = berry_lib_bytes(sets, n_links);
        TBK_CHECK(mesh_reserve(m->ws_mesh_work, off_lib + lib_bytes + 256, BERRY_FAMILY, "the workspace of the links"));
        char* q = m->ws_mesh_io.as<char>();
        double* d_L = reinterpret_cast<double*>(q);
        dev_words[(size_t)i] = reinterpret_cast<uint64_t*>(q + off_w);
        dev_abs[(size_t)i] = reinterpret_cast<double*>(q + off_a);
        double* d_D = convention == 1 ? reinterpret_cast<double*>(q + off_d) : nullptr;
        TBK_CHECK(res.upload(m));
        if (d_D) TBK_HIP(hipMemcpyAsync(d_D, h_D.data(), d_bytes, hipMemcpyHostToDevice, m->stream));
        TBK_CHECK(res.fill(m, true));
        TBK_CHECK(berry_launch_links(m->stream, m->blas, res.ev(), g, n_orb, sets, m->ws_mesh_u.as<double>(), d_D, k_lo, k_n,
                                     m->ws_mesh_work.as<char>() + off_lib, d_L, dev_words[(size_t)i], dev_abs[(size_t)i]));
    }
    tbk_model* m0 = handles[0];
    char* d_out = m0->ws_mesh_work.as<char>();
    const uint64_t* d_words = dev_words[0];
    const double* d_abs = dev_abs[0];
    if (!alone) {
        // synchronises every handle (the eigensolver's flags are reported as by tbk_eigh); the host puts the shares side by side
        TBK_CHECK(res.streams.check());
        try {
            h_words.resize(all_links);
            h_abs.resize(all_links);
            piece_w.resize((size_t)n_sets * dim * share.per);
            piece_a.resize(piece_w.size());
        } catch (...) {
            tbk_set_error("cannot allocate the words of the whole mesh");
            return TBK_ERR_MEMORY;
        }
        for (int i = 0; i < share.busy(); ++i) {
            const int64_t k_lo = share.lo(i), k_n = share.count(i);
            const size_t items = (size_t)n_sets * dim * k_n;
            TBK_HIP(hipSetDevice(handles[i]->device));
            TBK_HIP(hipMemcpy(piece_w.data(), dev_words[(size_t)i], items * sizeof(uint64_t), hipMemcpyDeviceToHost));
            TBK_HIP(hipMemcpy(piece_a.data(), dev_abs[(size_t)i], items * sizeof(double), hipMemcpyDeviceToHost));
            for (int r = 0; r < n_sets * dim; ++r) {
                std::memcpy(h_words.data() + (size_t)r * nk + k_lo, piece_w.data() + (size_t)r * k_n, (size_t)k_n * sizeof(uint64_t));
                std::memcpy(h_abs.data() + (size_t)r * nk + k_lo, piece_a.data() + (size_t)r * k_n, (size_t)k_n * sizeof(double));
            }
        }
        TBK_HIP(hipSetDevice(m0->device));
        uint64_t* all_w = reinterpret_cast<uint64_t*>(d_out + dos_align256(o.bytes));
        double* all_a = reinterpret_cast<double*>(d_out + dos_align256(o.bytes) + dos_align256(all_links * sizeof(uint64_t)));
        TBK_HIP(hipMemcpyAsync(all_w, h_words.data(), all_links * sizeof(uint64_t), hipMemcpyHostToDevice, m0->stream));
        TBK_HIP(hipMemcpyAsync(all_a, h_abs.data(), all_links * sizeof(double), hipMemcpyHostToDevice, m0->stream));
        d_words = all_w;
        d_abs = all_a;
    }
    TBK_HIP(hipSetDevice(m0->device));
    low.resize((size_t)n_sets * slices);
    TBK_CHECK(berry_launch_flux(m0->stream, &res.streams.used.front().ev, g, n_sets, slices, d_words, d_abs, o, d_out));
    TBK_HIP(hipMemcpyAsync(flux_out, d_out, (size_t)n_sets * planes * nk * sizeof(double), hipMemcpyDeviceToHost, m0->stream));
    TBK_HIP(hipMemcpyAsync(chern_out, d_out + o.off_chern, low.size() * sizeof(int64_t), hipMemcpyDeviceToHost, m0->stream));
    TBK_HIP(hipMemcpyAsync(low.data(), d_out + o.off_low, low.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, m0->stream));
    TBK_HIP(hipMemcpyAsync(link_min_out, d_out + o.off_min, (size_t)n_sets * sizeof(double), hipMemcpyDeviceToHost, m0->stream));
    // synchronises every handle (the eigensolver's flags are reported as by tbk_eigh) and books the kernel times
    TBK_CHECK(res.streams.finish(TIMED_BERRY));
    return berry_check_low(low);
}

extern "C" int tbk_berry_flux(tbk_model* m, const int32_t* mesh, int n_sets, const int32_t* ranges, int convention, const double* pos,
                              double* flux_out, int64_t* chern_out, double* link_min_out) {
    return tbk_berry_flux_multi(&m, 1, mesh, n_sets, ranges, convention, pos, flux_out, chern_out, link_min_out);
}

extern "C" int tbk_berry_timing(tbk_model* m, double* ms, int64_t* calls, int reset) {
    TBK_ARG(m != nullptr && ms != nullptr && calls != nullptr, "model / ms / calls is NULL");
    return tbk_timed_read(m, TIMED_BERRY, 3, ms, calls, nullptr, reset);
}
