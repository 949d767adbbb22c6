// tbk_surface.h -- what the kernels and launchers of tbk_surface.hip (the decimation, the transmission), tbk_ensemble.hip and
// tbk_channels.hip (the transmission of an ensemble of devices, its eigenvalues) and tbk_device_green.hip (the layer-resolved Green's
// functions of the device) share: the geometry of a workgroup's planes, the products, the iteration of the decimation,
// the layer body and the closing trace of the sweep, the constants, and the small inline helpers of the launchers.  The device
// templates sit in an unnamed namespace: each translation unit instantiates its own.  The host drivers of the whole calls, their
// helpers and surface_layers_kernel exist once, in tbk_layered.hip (tbk_layered.h).
#pragma once

#include <algorithm>
#include <cmath>
#include <type_traits>
#include <vector>

#include <rocsolver/rocsolver.h>

#include "tbk_resident.h"
#include "tbk_zmfma.h"

namespace {

constexpr int64_t SURF_MAX_Z = 4096;  // energies per call (include/tbk.h)
constexpr int SURF_OWN_MAX = 64;      // rows of a principal layer the decimation kernel takes
constexpr int SURF_LIB_MAX = 1024;    // ... and the library route above it (or on request)
constexpr int SURF_MAX_ITERATIONS = 4096;
constexpr unsigned long long SURF_NO_FLAG = ~0ull;
constexpr size_t SURF_CHUNK_BUDGET = size_t(256) << 20;  // the results of one chunk, and the H(k) samples of one chunk
constexpr double SURF_PI = 3.14159265358979323846;
constexpr const char* SURF_FAMILY = "the surface Green's function";

// What sits where, per template.  X, Y: two matrices in LDS, planes (re, im) of NP rows NP + 1 doubles apart -- the elimination runs
// in X, its un-permuted result g goes to Y, X then holds T.  alpha, beta, e, es, et: in LDS behind them up to NP = 32 (seven
// matrices), in the workgroup's slot of a global workspace at NP = 64 (pitch 64; the slot is reread by the workgroup that wrote
// it; 256 slots are 80 MiB: more than L2, inside the Infinity Cache).
template <int NP>
struct SurfGeom {
    static constexpr int THREADS = NP == 16 ? 64 : 256;
    static constexpr int WAVES = THREADS / 64;
    static constexpr int S = NP + 1;
    static constexpr int TR = NP / 16;               // tile rows
    static constexpr int NT = TR * TR / WAVES;       // 16 x 16 tiles of a product per wave: 1, 1, 4 (one tile row)
    static constexpr bool GLOBAL = NP == 64;
    static constexpr int SM = GLOBAL ? NP : S;       // pitch of alpha, beta, e, es, et
    static constexpr int LDS_PLANES = GLOBAL ? 4 : 14;
    static constexpr size_t lds_bytes = ((size_t)LDS_PLANES * NP * S + 2 * THREADS + 2 * NP + NP) * sizeof(double);
    static constexpr size_t slot_doubles = GLOBAL ? (size_t)10 * NP * NP : 0;
};

// The same integer, opaque to the optimiser and not to be moved out of a loop: offsets derived from it are computed where they are
// used.  Without it every address of the iteration's tiles -- 16 per plane, ten planes, 64 bits each at NP = 64 -- is hoisted in
// front of the item loop and the kernel spills: 2 800 bytes of scratch per thread at NP = 64 in the first build, which
// tests/test_dpp_hazards.py::test_no_product_kernel_spills reports.  If that test fails on this kernel after a
// compiler change, look here first.
__device__ __forceinline__ int surf_fresh(int x) {
    asm volatile("" : "+v"(x));
    return x;
}

// ---- the products -------------------------------------------------------------------------------------------------------------------
// C = op(A) op(B) of two NP x NP complex matrices in planes (pitches SA, SB), zero beyond n: the wave's NT tiles (tile row
// (wave NT) / TR, tile columns from (wave NT) % TR on) into registers.  Lane (q = lane / 16, c = lane % 16) feeds A[16 tr + c][k + q],
// B[k + q][16 tc + c] and holds C[16 tr + q + 4 r][16 tc + c], r = 0 ... 3.  AH: A^H in place of A, the fragment taken from A's
// columns and conjugated, conj(A[k + q][16 tr + c]); BH: B^H likewise, conj(B[16 tc + c][k + q]).  Tiles and K blocks beyond n are
// skipped (wave-uniform): they are zero.
template <int NP, int NT, int SA, int SB, bool AH = false, bool BH = false>
__device__ __forceinline__ void surf_product(const double* ar, const double* ai, const double* br, const double* bi, int n, int wave, int lane,
                                             zd4 (&cr)[NT], zd4 (&ci)[NT]) {
    constexpr int TR = NP / 16;
    lane = surf_fresh(lane);
    const int q = lane >> 4, c16 = lane & 15;
    const int tr = (wave * NT) / TR, tc0 = (wave * NT) % TR;
#pragma unroll
    for (int t = 0; t < NT; ++t) cr[t] = ci[t] = zd4{0.0, 0.0, 0.0, 0.0};
    if (tr * 16 >= n) return;
#pragma unroll 1
    for (int kb = 0; kb < TR; ++kb) {  // (not unrolled: the loads of every K block ahead of the first MFMA do not fit the registers)
        if (kb * 16 < n) {
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const int kk = kb * 16 + 4 * ks + q;
                const int ia = AH ? kk * SA + tr * 16 + c16 : (tr * 16 + c16) * SA + kk;
                const double a_r = ar[ia], a_i = AH ? -ai[ia] : ai[ia];
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    if ((tc0 + t) * 16 < n) {
                        const int ib = BH ? ((tc0 + t) * 16 + c16) * SB + kk : kk * SB + (tc0 + t) * 16 + c16;
                        const double b_r = br[ib], b_i = BH ? -bi[ib] : bi[ib];
                        zmfma_ab(a_r, a_i, b_r, b_i, cr[t], ci[t]);
                    }
                }
            }
        }
    }
}

// the wave's tiles of a product into a matrix (ADD: added to it); every element has one owner, whatever the matrix
template <int NP, int NT, int SD, bool ADD>
__device__ __forceinline__ void surf_tiles(double* dr, double* di, int n, int wave, int lane, const zd4 (&cr)[NT], const zd4 (&ci)[NT]) {
    constexpr int TR = NP / 16;
    lane = surf_fresh(lane);
    const int q = lane >> 4, c16 = lane & 15;
    const int tr = (wave * NT) / TR, tc0 = (wave * NT) % TR;
    if (tr * 16 >= n) return;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if ((tc0 + t) * 16 < n) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int at = (tr * 16 + q + 4 * r) * SD + (tc0 + t) * 16 + c16;
                if (ADD) {
                    dr[at] += cr[t][r];
                    di[at] += ci[t][r];
                } else {
                    dr[at] = cr[t][r];
                    di[at] = ci[t][r];
                }
            }
        }
    }
}

// |A|_inf and |B|_inf, row sums of |re| + |im| (the padding is zero): a thread sums NP / PARTS columns of its row, the first NP
// threads add the parts in order, every thread takes the maximum over the rows.  A NaN counts as +inf.  Two barriers inside; the
// matrices must be visible before the call.
template <int NP, int THREADS, int SM>
__device__ __forceinline__ void surf_norms(const double* ar, const double* ai, const double* br, const double* bi, int tid, double* red, double* rown,
                                           double& na, double& nb) {
    constexpr int PARTS = THREADS / NP, CPP = NP / PARTS;
    tid = surf_fresh(tid);
    const int row = tid & (NP - 1), part = tid / NP;
    double sa = 0.0, sb = 0.0;
#pragma unroll 4
    for (int cc = 0; cc < CPP; ++cc) {
        const int at = row * SM + part * CPP + cc;
        sa += fabs(ar[at]) + fabs(ai[at]);
        sb += fabs(br[at]) + fabs(bi[at]);
    }
    red[tid] = sa;
    red[THREADS + tid] = sb;
    __syncthreads();
    if (tid < NP) {
        double a = 0.0, b = 0.0;
#pragma unroll
        for (int p = 0; p < PARTS; ++p) {
            a += red[p * NP + tid];
            b += red[THREADS + p * NP + tid];
        }
        rown[tid] = a;
        rown[NP + tid] = b;
    }
    __syncthreads();
    na = 0.0;
    nb = 0.0;
#pragma unroll 4
    for (int r = 0; r < NP; ++r) {
        double a = rown[r], b = rown[NP + r];
        if (!(a <= DBL_MAX)) a = __builtin_inf();
        if (!(b <= DBL_MAX)) b = __builtin_inf();
        na = a > na ? a : na;
        nb = b > nb ? b : nb;
    }
}

// X = z 1 - M, zeros beyond n; jrow cleared for the elimination
template <int NP, int THREADS, int SM>
__device__ __forceinline__ void surf_form(double* xr, double* xi, const double* mr, const double* mi, double2 zz, int n, int tid, int* jrow) {
    constexpr int S = NP + 1;
    tid = surf_fresh(tid);
#pragma unroll 2
    for (int e = tid; e < NP * NP; e += THREADS) {
        const int i = e / NP, c = e - i * NP;
        double vr = 0.0, vi = 0.0;
        if (i < n && c < n) {
            vr = (i == c ? zz.x : 0.0) - mr[i * SM + c];
            vi = (i == c ? zz.y : 0.0) - mi[i * SM + c];
        }
        xr[i * S + c] = vr;
        xi[i * S + c] = vi;
    }
    if (tid < NP) jrow[tid] = -1;
}

// The planes of one workgroup (pitches: X, Y NP + 1; the others SurfGeom<NP>::SM) and its small tables.
struct SurfPlanes {
    double *xr, *xi, *yr, *yi;
    double *alr, *ali, *ber, *bei, *er, *ei, *esr, *esi, *etr, *eti;
    double* more;  // the matrices behind the five (the transmission's P)
    double *red, *rown;
    int *prow, *jrow;
};

// The planes of this workgroup: X and Y in LDS; MATS matrices (alpha, beta, e, es, et first) behind them up to NP = 32, in the
// workgroup's slot of ws at NP = 64; then the tables.
template <int NP, int MATS>
__device__ __forceinline__ SurfPlanes surf_planes(double* lds, double* ws) {
    using Geo = SurfGeom<NP>;
    constexpr int PX = NP * Geo::S, PM = NP * Geo::SM;
    SurfPlanes P;
    P.xr = lds;
    P.xi = P.xr + PX;
    P.yr = P.xi + PX;
    P.yi = P.yr + PX;
    double* mats;
    if constexpr (Geo::GLOBAL) {
        mats = ws + (size_t)blockIdx.x * ((size_t)2 * MATS * PM);
        P.red = P.yi + PX;
    } else {
        mats = P.yi + PX;
        P.red = mats + 2 * MATS * PM;
    }
    P.alr = mats;
    P.ali = mats + PM;
    P.ber = mats + 2 * PM;
    P.bei = mats + 3 * PM;
    P.er = mats + 4 * PM;
    P.ei = mats + 5 * PM;
    P.esr = mats + 6 * PM;
    P.esi = mats + 7 * PM;
    P.etr = mats + 8 * PM;
    P.eti = mats + 9 * PM;
    P.more = mats + 10 * PM;
    P.rown = P.red + 2 * Geo::THREADS;
    P.prow = reinterpret_cast<int*>(P.rown + 2 * NP);
    P.jrow = P.prow + NP;
    return P;
}

// es = et = e = H00, alpha = H01, beta = H01^H of one in-plane point into the planes, zeros beyond n (one barrier at the end)
template <int NP>
__device__ __forceinline__ void surf_load(const SurfPlanes& P, const double2* h0, const double2* h1, bool hops, int n, int tid) {
    using Geo = SurfGeom<NP>;
    constexpr int THREADS = Geo::THREADS, SM = Geo::SM;
    double *alr = P.alr, *ali = P.ali, *ber = P.ber, *bei = P.bei, *er = P.er, *ei = P.ei, *esr = P.esr, *esi = P.esi, *etr = P.etr, *eti = P.eti;
#pragma unroll 2
    for (int e = tid; e < NP * NP; e += THREADS) {
        const int i = e / NP, c = e - i * NP;
        double2 a = make_double2(0.0, 0.0), b = make_double2(0.0, 0.0);
        if (i < n && c < n) {
            a = h0[(size_t)i * n + c];
            if (hops) b = h1[(size_t)i * n + c];
        }
        er[i * SM + c] = esr[i * SM + c] = etr[i * SM + c] = a.x;
        ei[i * SM + c] = esi[i * SM + c] = eti[i * SM + c] = a.y;
        alr[i * SM + c] = b.x;
        ali[i * SM + c] = b.y;
        ber[c * SM + i] = b.x;
        bei[c * SM + i] = -b.y;
    }
    __syncthreads();
}

// The iteration of the header on loaded planes: the count into `it`, returns 0, 1 (singular) or 2 (the cap was reached), the same
// on every thread.  Afterwards es and et are final, alpha, beta, e, X and Y are free.
template <int NP>
__device__ __forceinline__ int surf_iterate(const SurfPlanes& P, double2 zz, int n, int max_it, int tid, int& it) {
    using Geo = SurfGeom<NP>;
    constexpr int THREADS = Geo::THREADS, S = Geo::S, SM = Geo::SM, NT = Geo::NT;
    const int lane = tid & 63, wave = tid >> 6;
    double *xr = P.xr, *xi = P.xi, *yr = P.yr, *yi = P.yi;
    double *alr = P.alr, *ali = P.ali, *ber = P.ber, *bei = P.bei, *er = P.er, *ei = P.ei, *esr = P.esr, *esi = P.esi, *etr = P.etr, *eti = P.eti;
    double *red = P.red, *rown = P.rown;
    int *prow = P.prow, *jrow = P.jrow;
    int status = 0;
    it = 0;
    double na, nb;
    surf_norms<NP, THREADS, SM>(alr, ali, ber, bei, tid, red, rown, na, nb);
    const double threshold = na * 0x1p-53;
    for (;;) {
        ++it;
        surf_form<NP, THREADS, SM>(xr, xi, er, ei, zz, n, tid, jrow);
        const bool zero_pivot = zgj_invert<NP, THREADS>(xr, xi, prow, jrow, n, tid);
        __syncthreads();
#pragma unroll 2
        for (int e = tid; e < NP * NP; e += THREADS) {  // g into Y, the permutations undone
            const int i = e / NP, c = e - i * NP;
            double vr = 0.0, vi = 0.0;
            if (i < n && c < n) {
                const int at = prow[i] * S + jrow[c];
                vr = xr[at];
                vi = xi[at];
            }
            yr[i * S + c] = vr;
            yi[i * S + c] = vi;
        }
        __syncthreads();
        zd4 tr[NT], ti[NT], p1r[NT], p1i[NT], p4r[NT], p4i[NT];
        surf_product<NP, NT, S, SM>(yr, yi, alr, ali, n, wave, lane, tr, ti);  // T = g alpha
        surf_tiles<NP, NT, S, false>(xr, xi, n, wave, lane, tr, ti);
        __syncthreads();
        surf_product<NP, NT, SM, S>(alr, ali, xr, xi, n, wave, lane, p1r, p1i);  // alpha g alpha
        surf_product<NP, NT, SM, S>(ber, bei, xr, xi, n, wave, lane, tr, ti);    // beta g alpha
        surf_tiles<NP, NT, SM, true>(etr, eti, n, wave, lane, tr, ti);
        surf_tiles<NP, NT, SM, true>(er, ei, n, wave, lane, tr, ti);
        __syncthreads();  // T has been read
        surf_product<NP, NT, S, SM>(yr, yi, ber, bei, n, wave, lane, tr, ti);  // T = g beta
        surf_tiles<NP, NT, S, false>(xr, xi, n, wave, lane, tr, ti);
        __syncthreads();
        surf_product<NP, NT, SM, S>(alr, ali, xr, xi, n, wave, lane, tr, ti);  // alpha g beta
        surf_tiles<NP, NT, SM, true>(esr, esi, n, wave, lane, tr, ti);
        surf_tiles<NP, NT, SM, true>(er, ei, n, wave, lane, tr, ti);
        surf_product<NP, NT, SM, S>(ber, bei, xr, xi, n, wave, lane, p4r, p4i);  // beta g beta
        __syncthreads();  // alpha and beta have been read
        surf_tiles<NP, NT, SM, false>(alr, ali, n, wave, lane, p1r, p1i);
        surf_tiles<NP, NT, SM, false>(ber, bei, n, wave, lane, p4r, p4i);
        __syncthreads();
        surf_norms<NP, THREADS, SM>(alr, ali, ber, bei, tid, red, rown, na, nb);
        const double size = na > nb ? na : nb;
        if (zero_pivot || !(size <= DBL_MAX)) {
            status = 1;
            break;
        }
        if (size <= threshold) break;
        if (it >= max_it) {
            status = 2;
            break;
        }
    }
    return status;
}

// ---- the transmission (tools/transport_model.py) ----------------------------------------------------------------
//   D_1 = et + V_1;  for p = 1 ... M:  (p = M: D_p += es - H00)  g_p = (z - D_p)^-1,  P_p = g_p (p = 1), g_p (H01^H P_{p-1}) (p > 1),
//   D_{p+1} = (H00 + V_{p+1}) + H01^H (g_p H01);   T = Re tr[(Gamma_R P_M) (Gamma_L P_M^H)],  Gamma = i (e - e^H) of es and et.
// After the decimation alpha, beta and e are dead: their planes take H01, H01^H (the prologue's loads again) and D; P is a sixth
// matrix behind et (LDS up to NP = 32: 140 032 bytes there; the slot of 12 planes at NP = 64).
template <int NP>
struct TransGeom {
    using Geo = SurfGeom<NP>;
    static constexpr int MATS = 6;
    static constexpr size_t lds_bytes = Geo::lds_bytes + (Geo::GLOBAL ? 0 : (size_t)2 * NP * Geo::S * sizeof(double));
    static constexpr size_t slot_doubles = Geo::GLOBAL ? (size_t)2 * MATS * NP * NP : 0;
};

// Element (i, c) of the potential of one layer in its two forms: a matrix [n][n] complex, or real on-site energies [n] (the ensemble,
// tbk_ensemble.hip) -- the energy on the diagonal and 0.0 elsewhere, so that the callers perform the additions of the matrix form on
// the expanded diagonal and give its bits.  trans_v_layer: the elements of one layer in the array.
__device__ __forceinline__ double2 trans_v(const double2* __restrict__ v, int i, int c, int n) { return v[(size_t)i * n + c]; }
__device__ __forceinline__ double2 trans_v(const double* __restrict__ v, int i, int c, int n) { return make_double2(i == c ? v[i] : 0.0, 0.0); }
__host__ __device__ __forceinline__ size_t trans_v_layer(const double2*, int n) { return (size_t)n * n; }
__host__ __device__ __forceinline__ size_t trans_v_layer(const double*, int n) { return (size_t)n; }

// the wave's tiles of a product into D = (H00 + V) + product (zero beyond n); h0, v: [n][n] in global memory (v: or [n]), read once
template <int NP, int NT, int SD, typename VT>
__device__ __forceinline__ void trans_tiles_onsite(double* dr, double* di, const double2* __restrict__ h0, const VT* __restrict__ v, int n, int wave,
                                                   int lane, const zd4 (&cr)[NT], const zd4 (&ci)[NT]) {
    constexpr int TR = NP / 16;
    lane = surf_fresh(lane);
    const int q = lane >> 4, c16 = lane & 15;
    const int tr = (wave * NT) / TR, tc0 = (wave * NT) % TR;
    if (tr * 16 >= n) return;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if ((tc0 + t) * 16 < n) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = tr * 16 + q + 4 * r, c = (tc0 + t) * 16 + c16;
                double vr = 0.0, vi = 0.0;
                if (i < n && c < n) {
                    const double2 a = h0[(size_t)i * n + c], b = trans_v(v, i, c, n);
                    vr = (a.x + b.x) + cr[t][r];
                    vi = (a.y + b.y) + ci[t][r];
                }
                dr[i * SD + c] = vr;
                di[i * SD + c] = vi;
            }
        }
    }
}

// the wave's tiles of a product into g [n][n] complex in global memory (rows and columns below n); one owner per element
template <int NP, int NT>
__device__ __forceinline__ void trans_tiles_stack(double2* g, int n, int wave, int lane, const zd4 (&cr)[NT], const zd4 (&ci)[NT]) {
    constexpr int TR = NP / 16;
    lane = surf_fresh(lane);
    const int q = lane >> 4, c16 = lane & 15;
    const int tr = (wave * NT) / TR, tc0 = (wave * NT) % TR;
    if (tr * 16 >= n) return;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if ((tc0 + t) * 16 < n) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = tr * 16 + q + 4 * r, c = (tc0 + t) * 16 + c16;
                if (i < n && c < n) g[(size_t)i * n + c] = make_double2(cr[t][r], ci[t][r]);
            }
        }
    }
}

// The sweep on the planes surf_iterate leaves (es and et final), shared by transmission_kernel and device_green_kernel
// (tbk_device_green.hip).  H01, H01^H and D live in the planes of alpha, beta and e, P in the sixth matrix.
// V: the potential in either form of trans_v.  trans_start: H01 and H01^H again; D_1 = et + V_1 (one barrier at the end)
template <int NP, typename VT>
__device__ __forceinline__ void trans_start(const SurfPlanes& P, const double2* __restrict__ h1, const VT* __restrict__ V, int n, int tid) {
    using Geo = SurfGeom<NP>;
    constexpr int THREADS = Geo::THREADS, SM = Geo::SM;
    double *h01r = P.alr, *h01i = P.ali, *h10r = P.ber, *h10i = P.bei, *dr = P.er, *di = P.ei, *etr = P.etr, *eti = P.eti;
#pragma unroll 2
    for (int e = tid; e < NP * NP; e += THREADS) {  // H01 and H01^H again; D_1 = et + V_1
        const int i = e / NP, c = e - i * NP;
        double2 b = make_double2(0.0, 0.0), d = make_double2(0.0, 0.0);
        if (i < n && c < n) {
            b = h1[(size_t)i * n + c];
            const double2 v = trans_v(V, i, c, n);
            d = make_double2(etr[i * SM + c] + v.x, eti[i * SM + c] + v.y);
        }
        h01r[i * SM + c] = b.x;
        h01i[i * SM + c] = b.y;
        h10r[c * SM + i] = b.x;
        h10i[c * SM + i] = -b.y;
        dr[i * SM + c] = d.x;
        di[i * SM + c] = d.y;
    }
    __syncthreads();
}

// Layer p (from 0) of the sweep: g_p into Y, P_p into P's planes, D_{p+1} into D's.  Returns whether a pivot was zero or an element
// of g_p not finite (this thread's share).  STACK: g_p goes to stack[2 p] and H01^H P_{p-1} (p > 0) to stack[2 p + 1], [n][n] complex
// each, by the threads that own the elements; a barrier stands between these stores and whatever the workgroup reads of them later.
template <int NP, bool STACK, typename VT>
__device__ __forceinline__ bool trans_layer(const SurfPlanes& P, const double2* __restrict__ h0, const VT* __restrict__ V, double2 zz, int p,
                                            int m_layers, int n, int tid, double2* stack) {
    using Geo = SurfGeom<NP>;
    constexpr int THREADS = Geo::THREADS, S = Geo::S, SM = Geo::SM, NT = Geo::NT;
    constexpr int PM = NP * SM;
    const int lane = tid & 63, wave = tid >> 6;
    double *xr = P.xr, *xi = P.xi, *yr = P.yr, *yi = P.yi;
    double *h01r = P.alr, *h01i = P.ali, *h10r = P.ber, *h10i = P.bei, *dr = P.er, *di = P.ei, *esr = P.esr, *esi = P.esi;
    double *pr = P.more, *pi = P.more + PM;
    int *prow = P.prow, *jrow = P.jrow;
    bool bad = false;
    if (p == m_layers - 1) {  // the right lead: D_M += es - H00 (the elements surf_form gives this thread)
#pragma unroll 2
        for (int e = tid; e < NP * NP; e += THREADS) {
            const int i = e / NP, c = e - i * NP;
            if (i < n && c < n) {
                const double2 a = h0[(size_t)i * n + c];
                dr[i * SM + c] += esr[i * SM + c] - a.x;
                di[i * SM + c] += esi[i * SM + c] - a.y;
            }
        }
    }
    surf_form<NP, THREADS, SM>(xr, xi, dr, di, zz, n, tid, jrow);
    bad |= zgj_invert<NP, THREADS>(xr, xi, prow, jrow, n, tid);
    __syncthreads();
#pragma unroll 2
    for (int e = tid; e < NP * NP; e += THREADS) {  // g_p into Y, the permutations undone
        const int i = e / NP, c = e - i * NP;
        double vr = 0.0, vi = 0.0;
        if (i < n && c < n) {
            const int at = prow[i] * S + jrow[c];
            vr = xr[at];
            vi = xi[at];
            bad |= !(fabs(vr) <= DBL_MAX && fabs(vi) <= DBL_MAX);
            if (STACK) stack[(size_t)2 * p * n * n + (size_t)i * n + c] = make_double2(vr, vi);
        }
        yr[i * S + c] = vr;
        yi[i * S + c] = vi;
        if (p == 0) {  // P_1 = g_1
            pr[i * SM + c] = vr;
            pi[i * SM + c] = vi;
        }
    }
    __syncthreads();
    zd4 cr[NT], ci[NT];
    if (p > 0) {
        surf_product<NP, NT, SM, SM>(h10r, h10i, pr, pi, n, wave, lane, cr, ci);  // T = H01^H P_{p-1}
        surf_tiles<NP, NT, S, false>(xr, xi, n, wave, lane, cr, ci);
        if (STACK) trans_tiles_stack<NP, NT>(stack + (size_t)(2 * p + 1) * n * n, n, wave, lane, cr, ci);
        __syncthreads();
        surf_product<NP, NT, S, S>(yr, yi, xr, xi, n, wave, lane, cr, ci);  // P_p = g_p T
        surf_tiles<NP, NT, SM, false>(pr, pi, n, wave, lane, cr, ci);
        __syncthreads();  // T has been read
    }
    if (p + 1 < m_layers) {
        surf_product<NP, NT, S, SM>(yr, yi, h01r, h01i, n, wave, lane, cr, ci);  // T = g_p H01
        surf_tiles<NP, NT, S, false>(xr, xi, n, wave, lane, cr, ci);
        __syncthreads();
        surf_product<NP, NT, SM, S>(h10r, h10i, xr, xi, n, wave, lane, cr, ci);  // H01^H g_p H01
        trans_tiles_onsite<NP, NT, SM>(dr, di, h0, V + (size_t)(p + 1) * trans_v_layer(V, n), n, wave, lane, cr, ci);
        __syncthreads();
    }
    return bad;
}

// The closing of the sweep: P_M is looked at (returns whether an element of this thread's share is not finite) and leaves to g_out
// unless that is NULL; T = Re tr[(Gamma_R P_M) (Gamma_L P_M^H)] and the count of the decimation go to *T_at and *it_at (it_at NULL:
// the count has another owner).  X, Y and D's planes are overwritten; P, es, et, H01 and H01^H stay.
template <int NP>
__device__ __forceinline__ bool trans_closing(const SurfPlanes& P, int n, int tid, double2* g_out, double* T_at, int32_t* it_at, int it) {
    using Geo = SurfGeom<NP>;
    constexpr int THREADS = Geo::THREADS, S = Geo::S, SM = Geo::SM, NT = Geo::NT;
    constexpr int PM = NP * SM;
    const int lane = tid & 63, wave = tid >> 6;
    double *xr = P.xr, *xi = P.xi, *yr = P.yr, *yi = P.yi;
    double *dr = P.er, *di = P.ei, *esr = P.esr, *esi = P.esi, *etr = P.etr, *eti = P.eti;
    double *pr = P.more, *pi = P.more + PM;
    double *red = P.red, *rown = P.rown;
    bool bad = false;
#pragma unroll 2
    for (int e = tid; e < NP * NP; e += THREADS) {  // Gamma_R into X, P_M^H into D's planes; P_M is looked at and leaves
        const int i = e / NP, c = e - i * NP;
        double gr = 0.0, gi = 0.0, ar = 0.0, ai = 0.0;
        if (i < n && c < n) {
            gr = -(esi[i * SM + c] + esi[c * SM + i]);
            gi = esr[i * SM + c] - esr[c * SM + i];
            ar = pr[c * SM + i];
            ai = -pi[c * SM + i];
            const double2 v = make_double2(pr[i * SM + c], pi[i * SM + c]);
            bad |= !(fabs(v.x) <= DBL_MAX && fabs(v.y) <= DBL_MAX);
            if (g_out != nullptr) g_out[(size_t)i * n + c] = v;
        }
        xr[i * S + c] = gr;
        xi[i * S + c] = gi;
        dr[i * SM + c] = ar;
        di[i * SM + c] = ai;
    }
    __syncthreads();
    {
        zd4 cr[NT], ci[NT];
        surf_product<NP, NT, S, SM>(xr, xi, pr, pi, n, wave, lane, cr, ci);  // Gamma_R P_M into Y
        surf_tiles<NP, NT, S, false>(yr, yi, n, wave, lane, cr, ci);
        __syncthreads();  // Gamma_R has been read
#pragma unroll 2
        for (int e = tid; e < NP * NP; e += THREADS) {  // Gamma_L into X
            const int i = e / NP, c = e - i * NP;
            double gr = 0.0, gi = 0.0;
            if (i < n && c < n) {
                gr = -(eti[i * SM + c] + eti[c * SM + i]);
                gi = etr[i * SM + c] - etr[c * SM + i];
            }
            xr[i * S + c] = gr;
            xi[i * S + c] = gi;
        }
        __syncthreads();
        surf_product<NP, NT, S, SM>(xr, xi, dr, di, n, wave, lane, cr, ci);  // Gamma_L P_M^H into X
        __syncthreads();  // Gamma_L has been read
        surf_tiles<NP, NT, S, false>(xr, xi, n, wave, lane, cr, ci);
        __syncthreads();
    }
    {
        // Re sum_ij Y[i][j] X[j][i] in a fixed order: a thread sums NP / PARTS columns of its row, the first NP threads add the
        // parts in order, thread 0 the rows
        constexpr int PARTS = THREADS / NP, CPP = NP / PARTS;
        const int row = tid & (NP - 1), part = tid / NP;
        double sum = 0.0;
#pragma unroll 4
        for (int cc = 0; cc < CPP; ++cc) {
            const int c = part * CPP + cc;
            if (row < n && c < n) sum += yr[row * S + c] * xr[c * S + row] - yi[row * S + c] * xi[c * S + row];
        }
        red[tid] = sum;
        __syncthreads();
        if (tid < NP) {
            double a = 0.0;
#pragma unroll
            for (int q = 0; q < PARTS; ++q) a += red[q * NP + tid];
            rown[tid] = a;
        }
        __syncthreads();
        if (tid == 0) {
            double total = 0.0;
#pragma unroll 4
            for (int r = 0; r < NP; ++r) total += rown[r];
            *T_at = total;
            if (it_at != nullptr) *it_at = it;
        }
        __syncthreads();  // the tables are free again
    }
    return bad;
}

// ---- host: what the launchers share (the drivers and their helpers: tbk_layered.h) ---------------------------------------------------
constexpr const char* TRANS_SINGULAR = "z - D of a device layer, or z - e of the decimation,";
constexpr int TRANS_MAX_LAYERS = 4096;
constexpr size_t TRANS_DEVICE_BUDGET = size_t(256) << 20;  // the device potential V [M][N][N] complex
constexpr size_t SURF_LDS_DEFAULT = size_t(64) << 10;      // dynamic LDS a kernel may ask for without tbk_raise_lds_limit

inline int64_t surf_grid(int n, int64_t items, int n_cu) {
    if (n > 32) return std::min<int64_t>(items, std::max(1, n_cu));  // one resident workgroup per CU, each with a workspace slot
    return std::min<int64_t>(items, int64_t(1) << 30);
}

inline bool surf_takes_library(int n, int eigensolver) { return n > SURF_OWN_MAX || eigensolver == TBK_EIG_ROCSOLVER; }

// The kernels' three sizes: f(std::integral_constant<int, NP>()) with the smallest NP that holds n rows.  Every *_launch_np<NP, ...>
// behind it keeps the flag row of its kernel as a local static and raises the LDS limit where its lds_bytes pass SURF_LDS_DEFAULT.
template <class F>
inline int surf_with_np(int n, F&& f) {
    if (n <= 16) return f(std::integral_constant<int, 16>());
    if (n <= 32) return f(std::integral_constant<int, 32>());
    return f(std::integral_constant<int, 64>());
}

}  // namespace
