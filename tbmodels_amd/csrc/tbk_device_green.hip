// tbk_device_green.hip -- the layer-resolved Green's functions of the device of tbk_transmission: the diagonal blocks G_pp of the
// resolvent with both lead self-energies attached, the blocks (p, 1) and (p, M), the local density of states per layer and orbital and
// its parts injected from each lead.  Not in the reference; DESIGN.md section 23 has the quantity, the kernel and the measurements,
// tools/device_model.py is the statement the tests compare with.
//
//   the decimation and the forward sweep of the transmission (tbk_surface.h): g_p, Q_p = G_{p,1} of the left-connected
//   system, T; then, with Gamma_R = i (es - es^H), Gamma_L = i (et - et^H),
//
//   G_M = g_M, C_M = g_M;  for p = M - 1 ... 1:  X = g_p H01, Y = H01^H g_p,  G_p = g_p + (X G_{p+1}) Y,  C_p = X C_{p+1}
//   F_1 = G_1,  F_p = G_p (H01^H Q_{p-1}) (1 < p < M),  F_M = Q_M (M > 1)
//   ldos[p][i] = -Im G_p[i][i] / pi,  left[p][i] = Re sum_j (F_p Gamma_L)[i][j] conj(F_p[i][j]) / (2 pi),  right: C_p and Gamma_R
//
//   device_green_kernel   one workgroup owns one (kp, z) from the first decimation step to the last output.  The forward sweep leaves
//                         g_p and H01^H Q_{p-1} of every layer on a stack of 2 M N^2 complex numbers in global memory, one stack per
//                         workgroup; the backward sweep reads it top down: eight products per layer on v_mfma_f64_16x16x4_f64.  The
//                         planes are the transmission's (D's take G_p, P's take C_p): no LDS beyond it.  N <= 64; there is no library
//                         route.
//
//   CURRENT (tbk_device_current*, DESIGN.md section 24, tools/current_model.py): the bond currents of the states injected from each lead,
//
//   K^L_p = 2 Im(conj(H01) o ((F_p Gamma_L) F_{p+1}^H)),  J^L_p = 2 Im(conj(H00 + V_p) o ((F_p Gamma_L) F_p^H)),  K^R, J^R: C_p and Gamma_R
//   current_left[p][i] = sum_j K^L_p[i][j],  current_right[p][i] = sum_j K^R_p[i][j]
//
//                         after each lead's row sums, when X still holds F_p Gamma_L (C_p Gamma_R): products A B^H (surf_product, BH) with
//                         the block of the layer above, which waits in the stack's dead place of g_{p+1} (H01^H Q_p), two more per layer
//                         and four when J is returned.  The false instantiation is the kernel above, statement for statement.

#include "tbk_layered.h"

namespace {

constexpr const char* DEVG_FAMILY = "the device Green's function";
constexpr const char* DEVG_SINGULAR = "z - D of a device layer, a block of the device's Green's function, or z - e of the decimation,";
constexpr const char* DEVC_SINGULAR =
    "z - D of a device layer, a block of the device's Green's function, a bond current, or z - e of the decimation,";
constexpr size_t DEVG_STACK_BUDGET = size_t(1) << 30;  // the workgroups' stacks of one launch: at M = 4096, N = 64 two still fit

// Re sum_j A[row][j] conj(B[row][j]) / (2 pi) for every row below n into out[row], in a fixed order: a thread sums NP / PARTS columns
// of its row, the first NP threads add the parts in order.  A: pitch NP + 1; B: pitch SB.  One barrier inside and one at the end.
template <int NP, int THREADS, int SB>
__device__ __forceinline__ void devg_row_sums(const double* ar, const double* ai, const double* br, const double* bi, int n, int tid, double* red,
                                              double* __restrict__ out) {
    constexpr int PARTS = THREADS / NP, CPP = NP / PARTS, S = NP + 1;
    tid = surf_fresh(tid);
    const int row = tid & (NP - 1), part = tid / NP;
    double sum = 0.0;
#pragma unroll 4
    for (int cc = 0; cc < CPP; ++cc) {
        const int c = part * CPP + cc;
        if (row < n && c < n) sum += ar[row * S + c] * br[row * SB + c] + ai[row * S + c] * bi[row * SB + c];
    }
    red[tid] = sum;
    __syncthreads();
    if (tid < NP && tid < n) {
        double a = 0.0;
#pragma unroll
        for (int q = 0; q < PARTS; ++q) a += red[q * NP + tid];
        out[tid] = a / (2.0 * SURF_PI);
    }
    __syncthreads();  // red and A are free again
}

// i (e - e^H) of the first n rows and columns of e (pitch SM) into X, zeros beyond
template <int NP, int THREADS, int SM>
__device__ __forceinline__ void devg_broadening(double* xr, double* xi, const double* er, const double* ei, int n, int tid) {
    constexpr int S = NP + 1;
    tid = surf_fresh(tid);
#pragma unroll 2
    for (int e = tid; e < NP * NP; e += THREADS) {
        const int i = e / NP, c = e - i * NP;
        double gr = 0.0, gi = 0.0;
        if (i < n && c < n) {
            gr = -(ei[i * SM + c] + ei[c * SM + i]);
            gi = er[i * SM + c] - er[c * SM + i];
        }
        xr[i * S + c] = gr;
        xi[i * S + c] = gi;
    }
}

// the wave's tiles of a product added to Y (pitch NP + 1) into D (pitch SD): D = Y + product
template <int NP, int NT, int SD>
__device__ __forceinline__ void devg_tiles_sum(double* dr, double* di, const double* yr, const double* yi, int n, int wave, int lane,
                                               const zd4 (&cr)[NT], const zd4 (&ci)[NT]) {
    constexpr int TR = NP / 16, S = NP + 1;
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
                dr[i * SD + c] = yr[i * S + c] + cr[t][r];
                di[i * SD + c] = yi[i * S + c] + ci[t][r];
            }
        }
    }
}

// ---- the bond currents (CURRENT; DESIGN.md section 24, tools/current_model.py) -----------------------------------------------------------
// What a layer's current step writes: rows of (M - 1) n doubles per item, bond matrices of (M - 1) n^2 and M n^2 (all four or none).
struct DevgCurrentOut {
    double *cur_l, *cur_r;      // current_left, current_right [items][M - 1][n]
    double *inter_l, *inter_r;  // K^L, K^R [items][M - 1][n][n] or NULL
    double *intra_l, *intra_r;  // J^L, J^R [items][M][n][n] or NULL
};

// sum_j A[row][j] for every row below n into out[row], in devg_row_sums' order.  A: one plane, pitch NP + 1.
template <int NP, int THREADS>
__device__ __forceinline__ void devg_row_totals(const double* a, int n, int tid, double* red, double* __restrict__ out) {
    constexpr int PARTS = THREADS / NP, CPP = NP / PARTS, S = NP + 1;
    tid = surf_fresh(tid);
    const int row = tid & (NP - 1), part = tid / NP;
    double sum = 0.0;
#pragma unroll 4
    for (int cc = 0; cc < CPP; ++cc) {
        const int c = part * CPP + cc;
        if (row < n && c < n) sum += a[row * S + c];
    }
    red[tid] = sum;
    __syncthreads();
    if (tid < NP && tid < n) {
        double t = 0.0;
#pragma unroll
        for (int q = 0; q < PARTS; ++q) t += red[q * NP + tid];
        out[tid] = t;
    }
    __syncthreads();  // red and A are free again
}

// 2 Im(conj(H[i][c]) A[i][c]) of the wave's tiles of A, by the lane that owns the element: into out [n][n] (not NULL) and, PLANE, into
// kr (pitch NP + 1).  H = h0 + v from global memory [n][n] (ONSITE) or from the planes hr, hi (pitch SH).  Returns whether an element of
// this thread's share is not finite.
template <int NP, int NT, int SH, bool ONSITE, bool PLANE>
__device__ __forceinline__ bool devg_tiles_bond(const double* hr, const double* hi, const double2* __restrict__ h0, const double2* __restrict__ v,
                                                double* kr, double* __restrict__ out, int n, int wave, int lane, const zd4 (&cr)[NT],
                                                const zd4 (&ci)[NT]) {
    constexpr int TR = NP / 16, S = NP + 1;
    lane = surf_fresh(lane);
    const int q = lane >> 4, c16 = lane & 15;
    const int tr = (wave * NT) / TR, tc0 = (wave * NT) % TR;
    bool bad = false;
    if (tr * 16 >= n) return bad;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if ((tc0 + t) * 16 < n) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = tr * 16 + q + 4 * r, c = (tc0 + t) * 16 + c16;
                double b = 0.0;
                if (i < n && c < n) {
                    double h_r, h_i;
                    if (ONSITE) {
                        const double2 a = h0[(size_t)i * n + c], w = v[(size_t)i * n + c];
                        h_r = a.x + w.x;
                        h_i = a.y + w.y;
                    } else {
                        h_r = hr[i * SH + c];
                        h_i = hi[i * SH + c];
                    }
                    b = 2.0 * (h_r * ci[t][r] - h_i * cr[t][r]);
                    bad |= !(fabs(b) <= DBL_MAX);
                    if (out != nullptr) out[(size_t)i * n + c] = b;
                }
                if (PLANE) kr[i * S + c] = b;
            }
        }
    }
    return bad;
}

// One lead's currents of layer p.  On entry X holds B_p Gamma (B = F: left, C: right) behind a barrier.  own: planes (pitch SO) that
// hold B_p, or NULL when Y already does; next: B_{p+1} [n][n] in the workgroup's stack, or NULL at the last layer.  J = 2 Im(conj(H00 +
// V_p) o (X Y^H)) goes to intra (not NULL), K = 2 Im(conj(H01) o (X B_{p+1}^H)) to inter (not NULL) and its row sums to cur.  X and Y
// are overwritten; ends behind a barrier.  Returns whether an element of K or J (this thread's share) is not finite.
template <int NP, int SO>
__device__ __forceinline__ bool devg_current_side(const SurfPlanes& P, const double* own_r, const double* own_i, const double2* next,
                                                  const double2* __restrict__ h0, const double2* __restrict__ vp, int n, int tid,
                                                  double* __restrict__ intra, double* __restrict__ inter, double* __restrict__ cur) {
    using Geo = SurfGeom<NP>;
    constexpr int THREADS = Geo::THREADS, S = Geo::S, SM = Geo::SM, NT = Geo::NT;
    const int lane = tid & 63, wave = tid >> 6;
    double *xr = P.xr, *xi = P.xi, *yr = P.yr, *yi = P.yi;
    bool bad = false;
    zd4 cr[NT], ci[NT];
    if (intra != nullptr) {
        if (own_r != nullptr) {
#pragma unroll 2
            for (int e = tid; e < NP * NP; e += THREADS) {  // B_p into Y
                const int i = e / NP, c = e - i * NP;
                yr[i * S + c] = own_r[i * SO + c];
                yi[i * S + c] = own_i[i * SO + c];
            }
            __syncthreads();
        }
        surf_product<NP, NT, S, S, false, true>(xr, xi, yr, yi, n, wave, lane, cr, ci);  // (B_p Gamma) B_p^H
        bad |= devg_tiles_bond<NP, NT, SM, true, false>(nullptr, nullptr, h0, vp, nullptr, intra, n, wave, lane, cr, ci);
        __syncthreads();  // Y has been read
    }
    if (next != nullptr) {
#pragma unroll 2
        for (int e = tid; e < NP * NP; e += THREADS) {  // B_{p+1} into Y
            const int i = e / NP, c = e - i * NP;
            double2 v = make_double2(0.0, 0.0);
            if (i < n && c < n) v = next[(size_t)i * n + c];
            yr[i * S + c] = v.x;
            yi[i * S + c] = v.y;
        }
        __syncthreads();
        surf_product<NP, NT, S, S, false, true>(xr, xi, yr, yi, n, wave, lane, cr, ci);  // (B_p Gamma) B_{p+1}^H
        __syncthreads();  // X has been read
        bad |= devg_tiles_bond<NP, NT, SM, false, true>(P.alr, P.ali, nullptr, nullptr, xr, inter, n, wave, lane, cr, ci);
        __syncthreads();
        devg_row_totals<NP, THREADS>(xr, n, tid, P.red, cur);
    }
    return bad;
}

// Layer p (from 0) of the backward sweep.  On entry (p < M - 1) D's planes hold G_{p+1} and P's C_{p+1}; at p = M - 1 P's hold Q_M as
// the forward sweep left it.  Afterwards D's hold G_p, P's C_p and Y F_p, and the layer's outputs are written.  stack: the
// workgroup's, as trans_layer wrote it.  Returns whether an element of G_p, F_p or C_p (this thread's share) is not finite.
// CURRENT: F_p and C_p take the stack's dead places of g_p and H01^H Q_{p-1}, written by the thread that looks at the element, and each
// lead's row sums are followed by devg_current_side; h0: H00 of the item, vp: V_p; co: the layer's places in the current outputs (K's
// and the rows are not touched at the last layer).  A non-finite element of K or J counts as one of the blocks.
template <int NP, bool CURRENT>
__device__ __forceinline__ bool devg_backward_layer(const SurfPlanes& P, double2* stack, int p, int m_layers, int n, int tid,
                                                    double* __restrict__ ldos, double* __restrict__ left, double* __restrict__ right,
                                                    double2* __restrict__ g_out, double2* __restrict__ f_out, double2* __restrict__ c_out,
                                                    const double2* __restrict__ h0, const double2* __restrict__ vp, const DevgCurrentOut& co) {
    using Geo = SurfGeom<NP>;
    constexpr int THREADS = Geo::THREADS, S = Geo::S, SM = Geo::SM, NT = Geo::NT;
    constexpr int PM = NP * SM;
    const int lane = tid & 63, wave = tid >> 6;
    double *xr = P.xr, *xi = P.xi, *yr = P.yr, *yi = P.yi;
    double *h01r = P.alr, *h01i = P.ali, *h10r = P.ber, *h10i = P.bei, *dr = P.er, *di = P.ei, *esr = P.esr, *esi = P.esi, *etr = P.etr, *eti = P.eti;
    double *pr = P.more, *pi = P.more + PM;
    double* red = P.red;
    const size_t nn = (size_t)n * n;
    double2* g = stack + (size_t)2 * p * nn;
    double2* hq = g + nn;  // H01^H Q_{p-1} (p > 0)
    bool bad = false;
    if (p == m_layers - 1) {
#pragma unroll 2
        for (int e = tid; e < NP * NP; e += THREADS) {  // F_M = Q_M into Y; G_M = C_M = g_M
            const int i = e / NP, c = e - i * NP;
            double2 v = make_double2(0.0, 0.0);
            if (i < n && c < n) v = g[(size_t)i * n + c];
            yr[i * S + c] = pr[i * SM + c];
            yi[i * S + c] = pi[i * SM + c];
            dr[i * SM + c] = pr[i * SM + c] = v.x;
            di[i * SM + c] = pi[i * SM + c] = v.y;
        }
        __syncthreads();
    } else {
#pragma unroll 2
        for (int e = tid; e < NP * NP; e += THREADS) {  // g_p into Y
            const int i = e / NP, c = e - i * NP;
            double2 v = make_double2(0.0, 0.0);
            if (i < n && c < n) v = g[(size_t)i * n + c];
            yr[i * S + c] = v.x;
            yi[i * S + c] = v.y;
        }
        __syncthreads();
        zd4 cr[NT], ci[NT], c2r[NT], c2i[NT];
        surf_product<NP, NT, S, SM>(yr, yi, h01r, h01i, n, wave, lane, cr, ci);  // X = g_p H01
        surf_tiles<NP, NT, S, false>(xr, xi, n, wave, lane, cr, ci);
        __syncthreads();
        surf_product<NP, NT, S, SM>(xr, xi, dr, di, n, wave, lane, cr, ci);    // X G_{p+1}
        surf_product<NP, NT, S, SM>(xr, xi, pr, pi, n, wave, lane, c2r, c2i);  // C_p = X C_{p+1}
        __syncthreads();  // X, G_{p+1} and C_{p+1} have been read
        surf_tiles<NP, NT, SM, false>(dr, di, n, wave, lane, cr, ci);
        surf_tiles<NP, NT, SM, false>(pr, pi, n, wave, lane, c2r, c2i);
        surf_product<NP, NT, SM, S>(h10r, h10i, yr, yi, n, wave, lane, cr, ci);  // Y = H01^H g_p, into X's planes
        surf_tiles<NP, NT, S, false>(xr, xi, n, wave, lane, cr, ci);
        __syncthreads();
        surf_product<NP, NT, SM, S>(dr, di, xr, xi, n, wave, lane, cr, ci);  // (X G_{p+1}) Y
        __syncthreads();  // X G_{p+1} has been read
        devg_tiles_sum<NP, NT, SM>(dr, di, yr, yi, n, wave, lane, cr, ci);  // G_p = g_p + (X G_{p+1}) Y
        if (p > 0) {
#pragma unroll 2
            for (int e = tid; e < NP * NP; e += THREADS) {  // H01^H Q_{p-1} into X
                const int i = e / NP, c = e - i * NP;
                double2 v = make_double2(0.0, 0.0);
                if (i < n && c < n) v = hq[(size_t)i * n + c];
                xr[i * S + c] = v.x;
                xi[i * S + c] = v.y;
            }
        }
        __syncthreads();  // G_p is whole, g_p has been read
        if (p > 0) {
            surf_product<NP, NT, SM, S>(dr, di, xr, xi, n, wave, lane, cr, ci);  // F_p = G_p (H01^H Q_{p-1})
            surf_tiles<NP, NT, S, false>(yr, yi, n, wave, lane, cr, ci);
        } else {
#pragma unroll 2
            for (int e = tid; e < NP * NP; e += THREADS) {  // F_1 = G_1
                const int i = e / NP, c = e - i * NP;
                yr[i * S + c] = dr[i * SM + c];
                yi[i * S + c] = di[i * SM + c];
            }
        }
        __syncthreads();
    }
    // the layer's blocks are looked at and leave; Gamma_L into X
    for (int e = tid; e < n * n; e += THREADS) {
        const int i = e / n, c = e - i * n;
        const double2 gv = make_double2(dr[i * SM + c], di[i * SM + c]), fv = make_double2(yr[i * S + c], yi[i * S + c]),
                      cv = make_double2(pr[i * SM + c], pi[i * SM + c]);
        bad |= !(fabs(gv.x) <= DBL_MAX && fabs(gv.y) <= DBL_MAX && fabs(fv.x) <= DBL_MAX && fabs(fv.y) <= DBL_MAX &&
                 fabs(cv.x) <= DBL_MAX && fabs(cv.y) <= DBL_MAX);
        if (g_out != nullptr) {
            g_out[e] = gv;
            f_out[e] = fv;
            c_out[e] = cv;
        }
        if constexpr (CURRENT) {  // g_p and H01^H Q_{p-1} have been read, behind barriers: layer p - 1 finds F_p and C_p there
            g[e] = fv;
            hq[e] = cv;
        }
        if (i == c) ldos[i] = -gv.y / SURF_PI;
    }
    devg_broadening<NP, THREADS, SM>(xr, xi, etr, eti, n, tid);
    __syncthreads();
    {
        zd4 cr[NT], ci[NT];
        surf_product<NP, NT, S, S>(yr, yi, xr, xi, n, wave, lane, cr, ci);  // F_p Gamma_L
        __syncthreads();  // Gamma_L has been read
        surf_tiles<NP, NT, S, false>(xr, xi, n, wave, lane, cr, ci);
        __syncthreads();
        devg_row_sums<NP, THREADS, S>(xr, xi, yr, yi, n, tid, red, left);
        if constexpr (CURRENT)
            bad |= devg_current_side<NP, S>(P, nullptr, nullptr, p + 1 < m_layers ? g + 2 * nn : nullptr, h0, vp, n, tid, co.intra_l, co.inter_l, co.cur_l);
        devg_broadening<NP, THREADS, SM>(xr, xi, esr, esi, n, tid);
        __syncthreads();
        surf_product<NP, NT, SM, S>(pr, pi, xr, xi, n, wave, lane, cr, ci);  // C_p Gamma_R
        __syncthreads();  // Gamma_R has been read
        surf_tiles<NP, NT, S, false>(xr, xi, n, wave, lane, cr, ci);
        __syncthreads();
        devg_row_sums<NP, THREADS, SM>(xr, xi, pr, pi, n, tid, red, right);
        if constexpr (CURRENT)
            bad |= devg_current_side<NP, SM>(P, pr, pi, p + 1 < m_layers ? hq + 2 * nn : nullptr, h0, vp, n, tid, co.intra_r, co.inter_r, co.cur_r);
    }
    return bad;
}

// H00, H01, V, z, items, key0, ws, iters, T_out, flag: transmission_kernel's.  stack: gridDim.x slots of slot_items = 2 m_layers n^2
// complex numbers; a slot is written and read by its workgroup alone.  Per item: ldos, left, right [m_layers][n] and, G_out not NULL,
// G_p, F_p, C_p [m_layers][n][n].  Status: a zero pivot or a non-finite element of a g_p, G_p, F_p or C_p is reason 0, the cap of
// the decimation reason 1; the sweeps run on after either.  Every branch is workgroup-uniform; no index depends on a value but through
// the pivot tables.  CURRENT: the bond currents as well (devg_backward_layer); co: the bases of their outputs.
template <int NP, bool CURRENT>
__global__ void __launch_bounds__(SurfGeom<NP>::THREADS)
    device_green_kernel(const double2* __restrict__ H00, const double2* __restrict__ H01, const double2* __restrict__ V, int m_layers,
                        const double2* __restrict__ z, int n_z, int n, int64_t items, int max_it, unsigned long long key0, double* ws, double2* stack,
                        size_t slot_items, int32_t* __restrict__ iters, double* __restrict__ T_out, double* __restrict__ ldos, double* __restrict__ left,
                        double* __restrict__ right, double2* __restrict__ G_out, double2* __restrict__ F_out, double2* __restrict__ C_out,
                        unsigned long long* __restrict__ flag, DevgCurrentOut co) {
    extern __shared__ double surf_lds[];
    const int tid = (int)threadIdx.x;
    const SurfPlanes P = surf_planes<NP, TransGeom<NP>::MATS>(surf_lds, ws);
    double2* st = stack + (size_t)blockIdx.x * slot_items;

    for (int64_t w = blockIdx.x; w < items; w += gridDim.x) {
        const int64_t k = w / n_z;
        const int zi = (int)(w - k * n_z);
        const double2 zz = z[zi];
        const double2* h0 = H00 + (size_t)k * n * n;
        const double2* h1 = H01 + (size_t)k * n * n;
        surf_load<NP>(P, h0, h1, true, n, tid);
        int it = 0;
        const int status = surf_iterate<NP>(P, zz, n, max_it, tid, it);  // 1: singular, 2: the cap (the same on every thread)
        bool bad = status == 1;
        trans_start<NP>(P, h1, V, n, tid);
#pragma unroll 1
        for (int p = 0; p < m_layers; ++p) bad |= trans_layer<NP, true>(P, h0, V, zz, p, m_layers, n, tid, st);
        bad |= trans_closing<NP>(P, n, tid, nullptr, T_out + w, iters + w, it);
        const size_t rows = ((size_t)w * m_layers) * n, mats = rows * n;
#pragma unroll 1
        for (int p = m_layers - 1; p >= 0; --p) {
            const size_t ro = rows + (size_t)p * n, mo = mats + (size_t)p * n * n;
            DevgCurrentOut at = co;
            if constexpr (CURRENT) {  // the layer's places; the last layer has no interface behind it
                const size_t rk = ((size_t)w * (m_layers - 1) + p) * n;
                at.cur_l += rk;
                at.cur_r += rk;
                if (co.intra_l != nullptr) {
                    at.inter_l += rk * n;
                    at.inter_r += rk * n;
                    at.intra_l += mo;
                    at.intra_r += mo;
                }
            }
            bad |= devg_backward_layer<NP, CURRENT>(P, st, p, m_layers, n, tid, ldos + ro, left + ro, right + ro, G_out != nullptr ? G_out + mo : nullptr,
                                                    G_out != nullptr ? F_out + mo : nullptr, G_out != nullptr ? C_out + mo : nullptr, h0,
                                                    V + (size_t)p * n * n, at);
        }
        const unsigned long long key = (key0 + (unsigned long long)k * (unsigned long long)SURF_MAX_Z + (unsigned long long)zi) * 2ull;
        if (bad) atomicMin(flag, key);
        if (status == 2 && tid == 0) atomicMin(flag, key + 1ull);
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
// The results of a chunk: T, iterations, ldos, left, right, (green) G, F, C, (current) current_left, current_right, (bonds) K^L, K^R,
// J^L, J^R, and behind them the status word.
struct DevgShape {
    int n = 0, m_layers = 0;
    int64_t n_z = 0;
    bool green = false;
    bool current = false, bonds = false;  // tbk_device_current*: the kernel's CURRENT instantiation; bonds needs current
    size_t t_bytes(int64_t nk) const { return dos_align256((size_t)nk * n_z * sizeof(double)); }
    size_t it_bytes(int64_t nk) const { return dos_align256((size_t)nk * n_z * sizeof(int32_t)); }
    size_t row_bytes(int64_t nk) const { return dos_align256((size_t)nk * n_z * m_layers * n * sizeof(double)); }
    size_t mat_bytes(int64_t nk) const { return green ? dos_align256((size_t)nk * n_z * m_layers * n * n * sizeof(double2)) : 0; }
    size_t cur_bytes(int64_t nk) const { return current ? dos_align256((size_t)nk * n_z * (m_layers - 1) * n * sizeof(double)) : 0; }
    size_t inter_bytes(int64_t nk) const { return bonds ? dos_align256((size_t)nk * n_z * (m_layers - 1) * n * n * sizeof(double)) : 0; }
    size_t intra_bytes(int64_t nk) const { return bonds ? dos_align256((size_t)nk * n_z * m_layers * n * n * sizeof(double)) : 0; }
    size_t result_bytes(int64_t nk) const {
        return t_bytes(nk) + it_bytes(nk) + 3 * row_bytes(nk) + 3 * mat_bytes(nk) + 2 * (cur_bytes(nk) + inter_bytes(nk) + intra_bytes(nk));
    }
    size_t slot_items() const { return (size_t)2 * m_layers * n * n; }  // complex numbers of one stack
    int64_t auto_chunk(int64_t nk) const {  // the chunk's results and its two layers inside the budget
        const size_t nn = (size_t)n * n * sizeof(double2);
        size_t per_item = sizeof(double) + sizeof(int32_t) + (size_t)m_layers * (3 * n * sizeof(double) + (green ? 3 * nn : 0));
        if (current) per_item += (size_t)(m_layers - 1) * 2 * n * sizeof(double);
        if (bonds) per_item += (size_t)(2 * m_layers - 1) * n * n * 2 * sizeof(double);
        const size_t per_k = (size_t)n_z * per_item + 2 * nn;
        return std::max<int64_t>(1, std::min<int64_t>(nk, (int64_t)(SURF_CHUNK_BUDGET / per_k)));
    }
};

// workgroups and stacks of a launch: the slots the budget holds, at most the items, the usual grid and the caller's cap (0: none)
int64_t devg_grid(const DevgShape& sh, int64_t items, int n_cu, int64_t slots) {
    int64_t grid = std::min<int64_t>(surf_grid(sh.n, items, n_cu), (int64_t)(DEVG_STACK_BUDGET / (sh.slot_items() * sizeof(double2))));
    if (slots > 0) grid = std::min(grid, slots);
    return std::max<int64_t>(1, grid);
}

size_t devg_stack_bytes(const DevgShape& sh, int64_t items, int n_cu, int64_t slots) {
    return (size_t)devg_grid(sh, items, n_cu, slots) * sh.slot_items() * sizeof(double2);
}

size_t devg_workspace_bytes(const DevgShape& sh, int64_t items, int n_cu, int64_t slots) {
    return sh.n > 32 ? (size_t)devg_grid(sh, items, n_cu, slots) * TransGeom<64>::slot_doubles * sizeof(double) : 0;
}

template <int NP, bool CURRENT>
int devg_launch_np(hipStream_t s, int n_cu, const DevgShape& sh, const double2* d_H00, const double2* d_H01, const double2* d_V, const double2* d_z,
                   int64_t nkc, int max_it, unsigned long long key0, int64_t slots, double* d_ws, double2* d_stack, char* d_res) {
    using Geo = SurfGeom<NP>;
    static tbk_flag_row done;  // of this instantiation's kernel
    const int64_t items = nkc * sh.n_z;
    if (TransGeom<NP>::lds_bytes > SURF_LDS_DEFAULT)
        TBK_HIP(tbk_raise_lds_limit(reinterpret_cast<const void*>(device_green_kernel<NP, CURRENT>), (int)TransGeom<NP>::lds_bytes, done));
    char* at = d_res;
    double* d_T = reinterpret_cast<double*>(at);
    at += sh.t_bytes(nkc);
    int32_t* d_it = reinterpret_cast<int32_t*>(at);
    at += sh.it_bytes(nkc);
    double* d_rows[3];
    for (int i = 0; i < 3; ++i, at += sh.row_bytes(nkc)) d_rows[i] = reinterpret_cast<double*>(at);
    double2* d_mats[3] = {nullptr, nullptr, nullptr};
    if (sh.green)
        for (int i = 0; i < 3; ++i, at += sh.mat_bytes(nkc)) d_mats[i] = reinterpret_cast<double2*>(at);
    double* d_cur[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // current_left, current_right, K^L, K^R, J^L, J^R
    if (sh.current)
        for (int i = 0; i < 2; ++i, at += sh.cur_bytes(nkc)) d_cur[i] = reinterpret_cast<double*>(at);
    if (sh.bonds) {
        for (int i = 2; i < 4; ++i, at += sh.inter_bytes(nkc)) d_cur[i] = reinterpret_cast<double*>(at);
        for (int i = 4; i < 6; ++i, at += sh.intra_bytes(nkc)) d_cur[i] = reinterpret_cast<double*>(at);
    }
    const DevgCurrentOut co = {d_cur[0], d_cur[1], d_cur[2], d_cur[3], d_cur[4], d_cur[5]};
    hipLaunchKernelGGL((device_green_kernel<NP, CURRENT>), dim3((unsigned)devg_grid(sh, items, n_cu, slots)), dim3(Geo::THREADS), TransGeom<NP>::lds_bytes, s, d_H00,
                       d_H01, d_V, sh.m_layers, d_z, (int)sh.n_z, sh.n, items, max_it, key0, d_ws, d_stack, sh.slot_items(), d_it, d_T, d_rows[0], d_rows[1],
                       d_rows[2], d_mats[0], d_mats[1], d_mats[2], reinterpret_cast<unsigned long long*>(d_res + sh.result_bytes(nkc)), co);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

// The chunk's nkc points at every energy.  d_res: DevgShape's layout for nkc points.
int devg_launch(hipStream_t s, int n_cu, const DevgShape& sh, const double2* d_H00, const double2* d_H01, const double2* d_V, const double2* d_z,
                int64_t nkc, int max_it, int64_t k0, int64_t slots, double* d_ws, double2* d_stack, char* d_res) {
    const unsigned long long key0 = (unsigned long long)k0 * (unsigned long long)SURF_MAX_Z;
    return surf_with_np(sh.n, [&](auto np) {
        constexpr int NP = decltype(np)::value;
        return sh.current ? devg_launch_np<NP, true>(s, n_cu, sh, d_H00, d_H01, d_V, d_z, nkc, max_it, key0, slots, d_ws, d_stack, d_res)
                          : devg_launch_np<NP, false>(s, n_cu, sh, d_H00, d_H01, d_V, d_z, nkc, max_it, key0, slots, d_ws, d_stack, d_res);
    });
}

// what the entry points check beyond the transmission's: the rows, the stack of one workgroup, the outputs
int devg_check(int N, int M, const double* ldos, const double* left, const double* right, const double* G, const double* F, const double* C) {
    if (N > SURF_OWN_MAX) {
        tbk_set_error("invalid argument: a principal layer of %d rows: the device Green's function takes at most %d", N, SURF_OWN_MAX);
        return TBK_ERR_ARGUMENT;
    }
    if ((size_t)2 * M * N * N * sizeof(double2) > DEVG_STACK_BUDGET) {
        tbk_set_error("invalid argument: a device of %d layers of %d rows: the stack of one workgroup may take at most 1 GiB", M, N);
        return TBK_ERR_ARGUMENT;
    }
    TBK_ARG(ldos != nullptr && left != nullptr && right != nullptr, "ldos / left / right is NULL");
    TBK_ARG((G != nullptr) == (F != nullptr) && (G != nullptr) == (C != nullptr), "G, F and C must all be NULL or none of them");
    return TBK_OK;
}

// ... and of the outputs of tbk_device_current*
int devg_check_current(const DevgCurrentOut& cur) {
    TBK_ARG(cur.cur_l != nullptr && cur.cur_r != nullptr, "current_left / current_right is NULL");
    const bool bonds = cur.inter_l != nullptr;
    TBK_ARG((cur.inter_r != nullptr) == bonds && (cur.intra_l != nullptr) == bonds && (cur.intra_r != nullptr) == bonds,
            "inter_left, inter_right, intra_left and intra_right must all be NULL or none of them");
    return TBK_OK;
}

// tbk_device_green* (cur NULL, timed on TIMED_DEVICE_GREEN) and tbk_device_current* (TIMED_DEVICE_CURRENT) behind the drivers of
// tbk_layered.h.  There is no library route: a handle with TBK_EIG_ROCSOLVER takes the own kernel too.  on_handle: the whole call on
// one handle looks at the outputs before the device, the kernel alone at the device first; slots: the option of *_from_matrices.
struct DevgFamily : LayeredFamily {
    DevgShape sh;
    bool on_handle;
    int64_t slots;
    int32_t* iterations;
    double *T, *ldos, *left, *right, *G, *F, *C;
    const DevgCurrentOut* cur;
    DevgFamily(bool on_handle_, int M, const double* V, int64_t n_z, int64_t slots_, int32_t* iterations_, double* T_, double* ldos_, double* left_,
               double* right_, double* G_, double* F_, double* C_, const DevgCurrentOut* cur_)
        : on_handle(on_handle_), slots(slots_), iterations(iterations_), T(T_), ldos(ldos_), left(left_), right(right_), G(G_), F(F_), C(C_), cur(cur_) {
        family = needs = DEVG_FAMILY;
        timed = cur != nullptr ? TIMED_DEVICE_CURRENT : TIMED_DEVICE_GREEN;
        rows_clamp = SURF_LIB_MAX;  // N > 64 is devg_check's to report, whatever N
        extra_what = "the workgroups' stacks";
        h_V = V;
        sh.m_layers = M;
        sh.n_z = n_z;
        sh.green = G != nullptr;
        sh.current = cur != nullptr;
        sh.bonds = cur != nullptr && cur->inter_l != nullptr;
    }
    int check(int N) override {
        sh.n = N;
        const double* V = static_cast<const double*>(h_V);
        if (!on_handle) TBK_CHECK(trans_check_device(N, sh.m_layers, V, iterations, T));
        TBK_CHECK(devg_check(N, on_handle ? std::max(sh.m_layers, 1) : sh.m_layers, ldos, left, right, G, F, C));
        if (cur != nullptr) TBK_CHECK(devg_check_current(*cur));
        if (on_handle) TBK_CHECK(trans_check_device(N, sh.m_layers, V, iterations, T));
        v_bytes = (size_t)sh.m_layers * N * N * sizeof(double2);
        return TBK_OK;
    }
    int check_options() const override {
        TBK_ARG(slots >= 0, "slots < 0");
        return TBK_OK;
    }
    size_t result_bytes(int64_t nk) const override { return sh.result_bytes(nk); }
    int64_t auto_chunk(int64_t nk) const override { return sh.auto_chunk(nk); }
    bool library(int) const override { return false; }
    size_t workspace_bytes(bool, int64_t chunk, int n_cu) const override { return devg_workspace_bytes(sh, chunk * sh.n_z, n_cu, slots); }
    size_t extra_bytes(int64_t chunk, int n_cu) const override { return devg_stack_bytes(sh, chunk * sh.n_z, n_cu, slots); }
    int run_chunk(bool, const LayeredChunk& c) const override {
        return devg_launch(c.s, c.n_cu, sh, c.d_H00, c.d_H01, static_cast<const double2*>(c.d_V), c.d_z, c.nkc, c.max_it, c.k0, slots,
                           reinterpret_cast<double*>(c.d_ws), reinterpret_cast<double2*>(c.d_extra), c.d_res);
    }
    int copy_out(const LayeredCopy& copy, const char* d_res, int64_t nkc, int64_t c0) const override {
        const size_t items = (size_t)nkc * sh.n_z, first = (size_t)c0 * sh.n_z;
        const size_t rows = (size_t)sh.m_layers * sh.n, mats = rows * sh.n * 2;
        const char* at = d_res;
        TBK_HIP(copy(T + first, at, items * sizeof(double)));
        at += sh.t_bytes(nkc);
        TBK_HIP(copy(iterations + first, at, items * sizeof(int32_t)));
        at += sh.it_bytes(nkc);
        double* row_out[3] = {ldos, left, right};
        for (int i = 0; i < 3; ++i, at += sh.row_bytes(nkc)) TBK_HIP(copy(row_out[i] + first * rows, at, items * rows * sizeof(double)));
        double* mat_out[3] = {G, F, C};
        if (sh.green)
            for (int i = 0; i < 3; ++i, at += sh.mat_bytes(nkc)) TBK_HIP(copy(mat_out[i] + first * mats, at, items * mats * sizeof(double)));
        if (sh.current) {
            const size_t krows = (size_t)(sh.m_layers - 1) * sh.n, kmats = krows * sh.n, jmats = rows * sh.n;
            double* cur_out[2] = {cur->cur_l, cur->cur_r};
            double* inter_out[2] = {cur->inter_l, cur->inter_r};
            double* intra_out[2] = {cur->intra_l, cur->intra_r};
            if (krows > 0)
                for (int i = 0; i < 2; ++i) TBK_HIP(copy(cur_out[i] + first * krows, at + i * sh.cur_bytes(nkc), items * krows * sizeof(double)));
            at += 2 * sh.cur_bytes(nkc);
            if (sh.bonds) {
                if (kmats > 0)
                    for (int i = 0; i < 2; ++i) TBK_HIP(copy(inter_out[i] + first * kmats, at + i * sh.inter_bytes(nkc), items * kmats * sizeof(double)));
                at += 2 * sh.inter_bytes(nkc);
                for (int i = 0; i < 2; ++i, at += sh.intra_bytes(nkc)) TBK_HIP(copy(intra_out[i] + first * jmats, at, items * jmats * sizeof(double)));
            }
        }
        return TBK_OK;
    }
    int status_error(unsigned long long word, const double* z, int max_iterations) const override {
        return surf_status_error(word, z, max_iterations, cur != nullptr ? DEVC_SINGULAR : DEVG_SINGULAR);
    }
};

}  // namespace

extern "C" int tbk_device_green_from_matrices(int device, int N, int64_t n_k, const double* H00, const double* H01, int M, const double* V, int64_t n_z,
                                              const double* z, int max_iterations, int64_t k_chunk, int64_t slots, int32_t* iterations, double* T,
                                              double* ldos, double* left, double* right, double* G, double* F, double* C) {
    DevgFamily fam(false, M, V, n_z, slots, iterations, T, ldos, left, right, G, F, C, nullptr);
    return layered_from_matrices(fam, device, N, n_k, H00, H01, n_z, z, max_iterations, k_chunk);
}

int tbk_device_green_slab(tbk_model* m, int64_t k_base, int axis, int layers, const double* k, int64_t nk, int M, const double* V, int64_t n_z,
                          const double* z, int max_iterations, int32_t* iterations, double* T, double* ldos, double* left, double* right, double* G,
                          double* F, double* C) {
    DevgFamily fam(true, M, V, n_z, 0, iterations, T, ldos, left, right, G, F, C, nullptr);
    return layered_slab(fam, m, k_base, axis, layers, k, nk, n_z, z, max_iterations);
}

extern "C" int tbk_device_green(tbk_model* m, int axis, int layers, const double* k, int64_t nk, int M, const double* V, int64_t n_z, const double* z,
                                int max_iterations, int32_t* iterations, double* T, double* ldos, double* left, double* right, double* G, double* F,
                                double* C) {
    return tbk_device_green_slab(m, 0, axis, layers, k, nk, M, V, n_z, z, max_iterations, iterations, T, ldos, left, right, G, F, C);
}

extern "C" int tbk_device_green_timing(tbk_model* m, double* ms, int64_t* calls, int reset) {
    TBK_ARG(m != nullptr && ms != nullptr && calls != nullptr, "model / ms / calls is NULL");
    return tbk_timed_read(m, TIMED_DEVICE_GREEN, 3, ms, calls, nullptr, reset);
}

// ---- the bond currents: the same calls with the kernel's CURRENT instantiation -----------------------------------
extern "C" int tbk_device_current_from_matrices(int device, int N, int64_t n_k, const double* H00, const double* H01, int M, const double* V, int64_t n_z,
                                                const double* z, int max_iterations, int64_t k_chunk, int64_t slots, int32_t* iterations, double* T,
                                                double* ldos, double* left, double* right, double* current_left, double* current_right,
                                                double* inter_left, double* inter_right, double* intra_left, double* intra_right) {
    const DevgCurrentOut cur = {current_left, current_right, inter_left, inter_right, intra_left, intra_right};
    DevgFamily fam(false, M, V, n_z, slots, iterations, T, ldos, left, right, nullptr, nullptr, nullptr, &cur);
    return layered_from_matrices(fam, device, N, n_k, H00, H01, n_z, z, max_iterations, k_chunk);
}

int tbk_device_current_slab(tbk_model* m, int64_t k_base, int axis, int layers, const double* k, int64_t nk, int M, const double* V, int64_t n_z,
                            const double* z, int max_iterations, int32_t* iterations, double* T, double* ldos, double* left, double* right,
                            double* current_left, double* current_right, double* inter_left, double* inter_right, double* intra_left,
                            double* intra_right) {
    const DevgCurrentOut cur = {current_left, current_right, inter_left, inter_right, intra_left, intra_right};
    DevgFamily fam(true, M, V, n_z, 0, iterations, T, ldos, left, right, nullptr, nullptr, nullptr, &cur);
    return layered_slab(fam, m, k_base, axis, layers, k, nk, n_z, z, max_iterations);
}

extern "C" int tbk_device_current(tbk_model* m, int axis, int layers, const double* k, int64_t nk, int M, const double* V, int64_t n_z, const double* z,
                                  int max_iterations, int32_t* iterations, double* T, double* ldos, double* left, double* right, double* current_left,
                                  double* current_right, double* inter_left, double* inter_right, double* intra_left, double* intra_right) {
    return tbk_device_current_slab(m, 0, axis, layers, k, nk, M, V, n_z, z, max_iterations, iterations, T, ldos, left, right, current_left, current_right,
                                   inter_left, inter_right, intra_left, intra_right);
}

extern "C" int tbk_device_current_timing(tbk_model* m, double* ms, int64_t* calls, int reset) {
    TBK_ARG(m != nullptr && ms != nullptr && calls != nullptr, "model / ms / calls is NULL");
    return tbk_timed_read(m, TIMED_DEVICE_CURRENT, 3, ms, calls, nullptr, reset);
}
