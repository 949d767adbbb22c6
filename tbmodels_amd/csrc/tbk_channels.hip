// tbk_channels.hip -- the transmission eigenvalues T_n of an ensemble of devices between the same two leads (DESIGN.md section 26,
// tools/channels_model.py): the eigenvalues of the matrix whose trace is tbk_transmission's T, from which the shot noise
// sum_n T_n (1 - T_n), the open channels and the distribution of the T_n follow.
//
//   transmission_channels_kernel<NP, DIAG>   transmission_ensemble_kernel's work items, decimation and sweep (tbk_ensemble.hip), unchanged
//                            and in its order -- T and iterations keep the bits of tbk_transmission -- and after trans_closing, per
//                            sample, chan_closing on the planes it left.  N <= 64; there is no library route.
//   chan_closing<NP>         B_R = s i (es - es^H) and B_L = s i (et - et^H), s = sign(Im z), into X and Y; both factored in place by
//                            chan_cholesky (diagonal pivoting on the vector unit, a rank-revealing stop); P_M L_L into D's planes and
//                            t = L_R^H (P_M L_L) on the FP64 matrix pipe; t -- t^H when the right lead has the smaller rank, so that
//                            the columns that are exactly zero stay columns -- into LDS over X and Y, column by column; the one-sided
//                            Jacobi of chan_jacobi; the squared column norms, sorted by rank counting, to the output.  It consumes X, Y,
//                            D and nothing else: P_M, es, et, H01 and H01^H stay for the next sample.
//
// The host is EnsFamily (tbk_ensemble.h) with this kernel as its route, behind the drivers of tbk_layered.h: the same chunks, staging
// and groups.

#include <type_traits>

#include "tbk_ensemble.h"

namespace {

constexpr int CHAN_MAX_SWEEPS = 48;  // MAX_SWEEPS of tools/channels_model.py: more than twice the 20 its inputs need
constexpr const char* CHAN_FAMILY = "the transmission eigenvalues";

// The Jacobi's view of a workgroup: a round's NP / 2 pairs take LPP lanes each (a power of two, inside one wave), a lane RPL rows of
// both columns.  t lies in LDS over X and Y by column, planes (re, im) of NP columns PT = NP + LPP doubles apart: the lanes of a pair
// read consecutive doubles, and PT = 24, 16, 8 (mod 32) puts the 32 / LPP pairs of a half wave, whose columns the round-robin order
// makes consecutive, on disjoint sets of LPP of the 32 double-wide banks -- a half wave's ds_read_b64 touches each bank once (but
// where a column index wraps around NP - 1).  A pitch of NP + 1, the other planes', would put column p + 1 one bank behind column p
// and four pairs onto eleven banks.
template <int NP>
struct ChanGeom {
    using Geo = SurfGeom<NP>;
    static constexpr int THREADS = Geo::THREADS;
    static constexpr int PAIRS = NP / 2;
    static constexpr int LPP = THREADS / PAIRS;  // 8, 16, 8
    static constexpr int RPL = NP / LPP;         // 2, 2, 8
    static constexpr int PT = NP + LPP;          // 24, 48, 72
    static_assert(LPP * PAIRS == THREADS && RPL * LPP == NP && (LPP & (LPP - 1)) == 0 && LPP <= 64, "a pair's lanes tile a wave");
    static_assert(2 * NP * PT <= 4 * NP * Geo::S, "t fits the four planes of X and Y");
    static_assert(2 * Geo::WAVES * (int)sizeof(int) <= 2 * THREADS * (int)sizeof(double), "the sweeps' flags fit red");
};

// B = sign i (e - e^H) of the planes e (pitch SM) into the planes b (pitch S), element by element as trans_closing forms Gamma; zeros
// beyond n.  taken[i] = -1 for the rows below n, NP beyond: the table of chan_cholesky.  No barrier inside.
template <int NP, int THREADS, int S, int SM>
__device__ __forceinline__ void chan_form(double* br, double* bi, const double* er, const double* ei, double sign, int n, int tid, int* taken) {
    tid = surf_fresh(tid);
#pragma unroll 2
    for (int e = tid; e < NP * NP; e += THREADS) {
        const int i = e / NP, c = e - i * NP;
        double gr = 0.0, gi = 0.0;
        if (i < n && c < n) {
            gr = sign * -(ei[i * SM + c] + ei[c * SM + i]);
            gi = sign * (er[i * SM + c] - er[c * SM + i]);
        }
        br[i * S + c] = gr;
        bi[i * S + c] = gi;
    }
    if (tid < NP) taken[tid] = tid < n ? -1 : NP;
}

// Cholesky with diagonal pivoting of a Hermitian positive semidefinite matrix in planes of pitch S, in place, one pivot per step, on
// the vector unit: `pivoted_cholesky` of tools/channels_model.py.  Step j takes the largest remaining diagonal (ties: the lowest index;
// a NaN counts as +inf), stops when it is <= n u d0 (d0: the first step's, u = 2^-53), writes its column of L into the pivot's own
// column p -- root at row p, 0.0 in the rows taken before, a[i][p] / root elsewhere -- and subtracts l_i conj(l_c) from what remains.
// Afterwards the columns no step took are cleared: B = L L^H over the columns, whatever their order.  taken: chan_form's table, the
// only index that depends on a value goes through it and through p.  (B as formed is exactly Hermitian; under FMA contraction the two
// triangles of the remainder stop being exact conjugates and its diagonal picks up a rounding-sized imaginary part -- only Re of the
// diagonal and column p are read, so this stays a rounding-level difference from the model.)  Returns the rank (the same on every
// thread); the planes must be written before the call (its first barrier orders them) and are complete behind a barrier of the
// caller's.
template <int NP, int THREADS, int S>
__device__ __forceinline__ int chan_cholesky(double* ar, double* ai, int* taken, int n, int tid) {
    constexpr int EPT = NP * NP / THREADS;  // elements per thread: its column c = tid % NP, rows tid / NP + e THREADS / NP
    constexpr int RSTEP = THREADS / NP;
    tid = surf_fresh(tid);
    const int c = tid & (NP - 1), r0 = tid / NP;
    bool used = c >= n;
    double threshold = 0.0;
    int rank = 0;
#pragma unroll 1
    for (int j = 0; j < n; ++j) {
        __syncthreads();  // what remains is up to date
        double best = ar[c * S + c];
        if (best != best) best = __builtin_inf();
        if (used) best = -__builtin_inf();
        int p = c;
#pragma unroll
        for (int off = NP / 2; off > 0; off >>= 1) {
            const double ob = __shfl_xor(best, off, 64);
            const int op = __shfl_xor(p, off, 64);
            if (ob > best || (ob == best && op < p)) {
                best = ob;
                p = op;
            }
        }
        if (j == 0) threshold = (double)n * 0x1p-53 * best;
        if (best <= threshold) break;  // (every thread holds the same best: the branch is workgroup-uniform)
        rank = j + 1;
        const double inv = 1.0 / sqrt(best);
        const double lcr = ar[c * S + p] * inv, lci = ai[c * S + p] * inv;  // l_c
        double nr[EPT], ni[EPT];
        bool write[EPT];
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int i = r0 + e * RSTEP;
            const bool gone = taken[i] >= 0;  // row i was taken before this step (or lies beyond n)
            const double lir = ar[i * S + p] * inv, lii = ai[i * S + p] * inv;  // l_i
            const double vr = ar[i * S + c], vi = ai[i * S + c];
            if (c == p) {  // the column of L
                nr[e] = gone ? 0.0 : (i == p ? sqrt(best) : lir);
                ni[e] = gone || i == p ? 0.0 : lii;
                write[e] = true;
            } else {
                nr[e] = vr - (lir * lcr + lii * lci);
                ni[e] = vi - (lii * lcr - lir * lci);
                write[e] = !gone && !used && i != p;
            }
        }
        __syncthreads();  // column p and the table have been read
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int i = r0 + e * RSTEP;
            if (write[e]) {
                ar[i * S + c] = nr[e];
                ai[i * S + c] = ni[e];
            }
        }
        if (c == p) {
            used = true;
            if (r0 == 0) taken[p] = j;
        }
    }
    __syncthreads();  // the last step's stores; every thread is out of the loop
    if (!used) {      // a column below n that no step took
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int i = r0 + e * RSTEP;
            ar[i * S + c] = 0.0;
            ai[i * S + c] = 0.0;
        }
    }
    return rank;
}

// One-sided (Hestenes) Jacobi on the NP columns of t in LDS (ChanGeom's layout): `hestenes` of tools/channels_model.py.  A sweep is
// NP - 1 rounds of NP / 2 disjoint pairs in the round-robin order -- pair 0 of round r is (r, NP - 1), pair j >= 1 is
// ((r + j) mod (NP - 1), (r - j) mod (NP - 1)) -- one barrier per round.  A pair's LPP lanes sum a = |t_p|^2, b = |t_q|^2 and
// c = t_p^H t_q over their rows in ascending order and then across the lanes by a butterfly, so every lane holds the same bits; the
// rotation is applied by selects, there is no branch on a value.  A wave's rotations of a sweep meet in LDS (flags, two sets taken in
// turn) before the sweep's last barrier, so the exit is workgroup-uniform.  Returns whether CHAN_MAX_SWEEPS sweeps all rotated.
template <int NP>
__device__ __forceinline__ bool chan_jacobi(double* tr, double* ti, int* flags, int n, int tid) {
    using CG = ChanGeom<NP>;
    constexpr int LPP = CG::LPP, RPL = CG::RPL, PT = CG::PT, WAVES = CG::Geo::WAVES;
    tid = surf_fresh(tid);
    const int pair = tid / LPP, l = tid & (LPP - 1), lane = tid & 63, wave = tid >> 6;
    const double limit = (double)n * 0x1p-53;
    bool capped = false;
#pragma unroll 1
    for (int sweep = 0;; ++sweep) {
        bool rotated = false;
#pragma unroll 1
        for (int r = 0; r < NP - 1; ++r) {
            int u = r + pair, v = r - pair;
            if (u >= NP - 1) u -= NP - 1;
            if (v < 0) v += NP - 1;
            if (pair == 0) v = NP - 1;
            const int p = u < v ? u : v, q = u < v ? v : u;
            double xr[RPL], xi[RPL], yr[RPL], yi[RPL];
            double a = 0.0, b = 0.0, cr = 0.0, ci = 0.0;
#pragma unroll
            for (int k = 0; k < RPL; ++k) {
                const int row = l + LPP * k;
                xr[k] = tr[p * PT + row];
                xi[k] = ti[p * PT + row];
                yr[k] = tr[q * PT + row];
                yi[k] = ti[q * PT + row];
                a += xr[k] * xr[k] + xi[k] * xi[k];
                b += yr[k] * yr[k] + yi[k] * yi[k];
                cr += xr[k] * yr[k] + xi[k] * yi[k];
                ci += xr[k] * yi[k] - xi[k] * yr[k];
            }
#pragma unroll
            for (int off = LPP / 2; off > 0; off >>= 1) {
                a += __shfl_xor(a, off, 64);
                b += __shfl_xor(b, off, 64);
                cr += __shfl_xor(cr, off, 64);
                ci += __shfl_xor(ci, off, 64);
            }
            const double size = hypot(cr, ci);
            const bool go = a != 0.0 && b != 0.0 && size > limit * sqrt(a) * sqrt(b);  // (a NaN: no rotation)
            const double zeta = (b - a) / (2.0 * size);
            const double tau = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
            const double cs = 1.0 / sqrt(1.0 + tau * tau), sn = cs * tau;
            const double wr = sn * (cr / size), wi = sn * (ci / size);
            rotated |= go;
#pragma unroll
            for (int k = 0; k < RPL; ++k) {
                const int row = l + LPP * k;
                // t_p' = cs t_p - conj(w) t_q,  t_q' = w t_p + cs t_q
                const double pr = cs * xr[k] - (wr * yr[k] + wi * yi[k]), pi = cs * xi[k] - (wr * yi[k] - wi * yr[k]);
                const double qr = (wr * xr[k] - wi * xi[k]) + cs * yr[k], qi = (wr * xi[k] + wi * xr[k]) + cs * yi[k];
                tr[p * PT + row] = go ? pr : xr[k];
                ti[p * PT + row] = go ? pi : xi[k];
                tr[q * PT + row] = go ? qr : yr[k];
                ti[q * PT + row] = go ? qi : yi[k];
            }
            if (r == NP - 2) {  // the sweep's rotations of this wave, ahead of its last barrier
                const bool any = __any(rotated ? 1 : 0) != 0;
                if (lane == 0) flags[(sweep & 1) * WAVES + wave] = any ? 1 : 0;
            }
            __syncthreads();  // the round's columns are written
        }
        int any = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) any |= flags[(sweep & 1) * WAVES + w];
        if (any == 0) break;
        if (sweep + 1 >= CHAN_MAX_SWEEPS) {
            capped = true;
            break;
        }
    }
    return capped;
}

// The closing of a sample behind trans_closing: the n transmission eigenvalues, descending, to out[0 ... n).  sign: of Im z.  Returns
// whether the Jacobi reached its cap (the same on every thread); bad: set on the thread that finds a squared norm that is not finite
// (an overflow in a broadening or in t that trans_closing's look at P_M does not see) -- the rank counting cannot order such values,
// out[] is then incomplete and the caller raises the sample's status.  X, Y and D's planes are overwritten; P, es, et, H01 and H01^H stay.
template <int NP>
__device__ __forceinline__ bool chan_closing(const SurfPlanes& P, double sign, int n, int tid, double* __restrict__ out, bool& bad) {
    using Geo = SurfGeom<NP>;
    using CG = ChanGeom<NP>;
    constexpr int THREADS = Geo::THREADS, S = Geo::S, SM = Geo::SM, NT = Geo::NT, PT = CG::PT, TR = NP / 16;
    constexpr int PM = NP * SM;
    const int lane = tid & 63, wave = tid >> 6;
    double *xr = P.xr, *xi = P.xi, *yr = P.yr, *yi = P.yi;
    double *dr = P.er, *di = P.ei;
    double *pr = P.more, *pi = P.more + PM;
    double *tr = P.xr, *ti = P.xr + NP * PT;  // t, over X and Y once L_R and L_L are dead
    chan_form<NP, THREADS, S, SM>(xr, xi, P.esr, P.esi, sign, n, tid, P.jrow);
    const int rank_r = chan_cholesky<NP, THREADS, S>(xr, xi, P.jrow, n, tid);  // L_R in X
    __syncthreads();  // the table is free
    chan_form<NP, THREADS, S, SM>(yr, yi, P.etr, P.eti, sign, n, tid, P.jrow);
    const int rank_l = chan_cholesky<NP, THREADS, S>(yr, yi, P.jrow, n, tid);  // L_L in Y
    __syncthreads();
    {
        zd4 cr[NT], ci[NT];
        surf_product<NP, NT, SM, S>(pr, pi, yr, yi, n, wave, lane, cr, ci);  // P_M L_L into D
        surf_tiles<NP, NT, SM, false>(dr, di, n, wave, lane, cr, ci);
        __syncthreads();
        surf_product<NP, NT, S, SM, true, false>(xr, xi, dr, di, n, wave, lane, cr, ci);  // t = L_R^H (P_M L_L)
        __syncthreads();  // L_R and L_L have been read
        // every tile of t, the zero ones beyond n included, into the Jacobi's columns: t as it is when r_L <= r_R, else t^H
        const bool flip = rank_l > rank_r;  // (uniform)
        const int q = surf_fresh(lane) >> 4, c16 = lane & 15;
        const int trow = (wave * NT) / TR, tc0 = (wave * NT) % TR;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = trow * 16 + q + 4 * r, c = (tc0 + t) * 16 + c16;
                const int at = flip ? i * PT + c : c * PT + i;
                tr[at] = cr[t][r];
                ti[at] = flip ? -ci[t][r] : ci[t][r];
            }
        }
        __syncthreads();
    }
    const bool capped = chan_jacobi<NP>(tr, ti, reinterpret_cast<int*>(P.red), n, tid);
    // (chan_jacobi ends behind a barrier)  the squared column norms, rows ascending; then the rank of each among all
    if (tid < NP) {
        double v = 0.0;
#pragma unroll 4
        for (int i = 0; i < NP; ++i) v += tr[tid * PT + i] * tr[tid * PT + i] + ti[tid * PT + i] * ti[tid * PT + i];
        P.rown[tid] = v;
        bad |= !(v <= DBL_MAX);
    }
    __syncthreads();
    if (tid < NP) {
        const double v = P.rown[tid];
        int rank = 0;
#pragma unroll 4
        for (int j = 0; j < NP; ++j) {
            const double o = P.rown[j];
            rank += (o > v || (o == v && j < tid)) ? 1 : 0;
        }
        if (rank < n) out[rank] = v;  // (the columns beyond n are zero and follow every zero column below n)
    }
    __syncthreads();  // the planes and the tables are free again
    return capped;
}

// transmission_ensemble_kernel's arguments, and ch_out: [nkc][n_z][n_s][n].  The status word takes the smallest
// (((point index * SURF_MAX_Z + energy index) * ENS_MAX_SAMPLES + sample) * 4 + reason): reasons 0 and 1 as in the ensemble's kernel
// (0 also for a T_n that is not finite), reason 2 the cap of the Jacobi with that sample.  Every branch is workgroup-uniform; no index depends on a value but through the
// pivot tables; plain vector stores, one owner per output; a workgroup reads only its own slot.
template <int NP, bool DIAG>
__global__ void __launch_bounds__(SurfGeom<NP>::THREADS)
    transmission_channels_kernel(const double2* __restrict__ H00, const double2* __restrict__ H01, const void* __restrict__ V, int m_layers, int n_s, int spg,
                                 int groups, const double2* __restrict__ z, int n_z, int n, int64_t items, int max_it, unsigned long long key0, double* ws,
                                 int32_t* __restrict__ iters, double* __restrict__ T_out, double* __restrict__ ch_out,
                                 unsigned long long* __restrict__ flag) {
    using VT = typename std::conditional<DIAG, double, double2>::type;
    extern __shared__ double surf_lds[];
    const int tid = (int)threadIdx.x;
    const SurfPlanes P = surf_planes<NP, TransGeom<NP>::MATS>(surf_lds, ws);
    const size_t per_sample = (size_t)m_layers * trans_v_layer(static_cast<const VT*>(nullptr), n);

    for (int64_t w = blockIdx.x; w < items; w += gridDim.x) {
        const int64_t kz = w / groups;
        const int g = (int)(w - kz * groups);
        const int64_t k = kz / n_z;
        const int zi = (int)(kz - k * n_z);
        const double2 zz = z[zi];
        const double sign = zz.y > 0.0 ? 1.0 : -1.0;
        const double2* h0 = H00 + (size_t)k * n * n;
        const double2* h1 = H01 + (size_t)k * n * n;
        surf_load<NP>(P, h0, h1, true, n, tid);
        int it = 0;
        const int status = surf_iterate<NP>(P, zz, n, max_it, tid, it);  // 1: singular, 2: the cap (the same on every thread)
        const unsigned long long key =
            (key0 + (unsigned long long)k * (unsigned long long)SURF_MAX_Z + (unsigned long long)zi) * (unsigned long long)ENS_MAX_SAMPLES;
        const int s0 = g * spg, s1 = s0 + spg < n_s ? s0 + spg : n_s;
#pragma unroll 1
        for (int s = s0; s < s1; ++s) {
            const VT* Vs = static_cast<const VT*>(V) + (size_t)s * per_sample;
            bool bad = status == 1;
            trans_start<NP>(P, h1, Vs, n, tid);
#pragma unroll 1
            for (int p = 0; p < m_layers; ++p) bad |= trans_layer<NP, false>(P, h0, Vs, zz, p, m_layers, n, tid, nullptr);
            bad |= trans_closing<NP>(P, n, tid, nullptr, T_out + (size_t)kz * n_s + s, s == 0 ? iters + kz : nullptr, it);
            const bool capped = chan_closing<NP>(P, sign, n, tid, ch_out + ((size_t)kz * n_s + s) * n, bad);
            if (bad) atomicMin(flag, (key + (unsigned long long)s) * 4ull);
            if (capped && tid == 0) atomicMin(flag, (key + (unsigned long long)s) * 4ull + 2ull);
        }
        if (status == 2 && g == 0 && tid == 0) atomicMin(flag, key * 4ull + 1ull);
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
template <int NP, bool DIAG>
int chan_launch_np(const EnsShape& sh, const EnsLaunch& a) {
    using Geo = SurfGeom<NP>;
    static tbk_flag_row done;  // of this instantiation's kernel
    const void* kernel = reinterpret_cast<const void*>(transmission_channels_kernel<NP, DIAG>);
    if (TransGeom<NP>::lds_bytes > SURF_LDS_DEFAULT) TBK_HIP(tbk_raise_lds_limit(kernel, (int)TransGeom<NP>::lds_bytes, done));
    int64_t spg = 0, groups = 0;
    TBK_CHECK(ens_sample_groups<NP>(kernel, sh, a, spg, groups));  // the ensemble's rule: the dynamic LDS, and so the occupancy, are its kernel's
    const int64_t items = a.nkc * sh.n_z * groups;
    hipLaunchKernelGGL((transmission_channels_kernel<NP, DIAG>), dim3((unsigned)surf_grid(sh.n, items, a.n_cu)), dim3(Geo::THREADS), TransGeom<NP>::lds_bytes,
                       a.s, a.d_H00, a.d_H01, a.d_V, sh.m_layers, (int)sh.n_s, (int)spg, (int)groups, a.d_z, (int)sh.n_z, sh.n, items, a.max_it, a.key0,
                       a.d_ws, a.d_it, a.d_T, a.d_ch, a.d_flag);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

// The chunk's nkc points at every energy and sample (N <= 64: the drivers have checked it)
int chan_launch(const EnsShape& sh, const EnsLaunch& a) {
    return surf_with_np(sh.n, [&](auto np) {
        return sh.diag ? chan_launch_np<decltype(np)::value, true>(sh, a) : chan_launch_np<decltype(np)::value, false>(sh, a);
    });
}

const EnsRoute CHAN_ROUTE = {chan_launch, 4u, true, TIMED_TRANSMISSION_CHANNELS, CHAN_FAMILY};

}  // namespace

extern "C" int tbk_transmission_channels_from_matrices(int device, int N, int64_t n_k, const double* H00, const double* H01, int M, int64_t n_s,
                                                       const double* V, const double* onsite, int64_t n_z, const double* z, int max_iterations,
                                                       int64_t k_chunk, int64_t sample_chunk, int32_t* iterations, double* T, double* channels) {
    EnsFamily fam(CHAN_ROUTE, M, n_s, V, onsite, n_z, sample_chunk, iterations, T, channels);
    return layered_from_matrices(fam, device, N, n_k, H00, H01, n_z, z, max_iterations, k_chunk);
}

// The whole call on one handle; k_base as in tbk_surface_green_slab
int tbk_transmission_channels_slab(tbk_model* m, int64_t k_base, int axis, int layers, const double* k, int64_t nk, int M_device, int64_t n_s,
                                   const double* V, const double* onsite, int64_t n_z, const double* z, int max_iterations, int32_t* iterations, double* T,
                                   double* channels) {
    EnsFamily fam(CHAN_ROUTE, M_device, n_s, V, onsite, n_z, 0, iterations, T, channels);
    return layered_slab(fam, m, k_base, axis, layers, k, nk, n_z, z, max_iterations);
}

extern "C" int tbk_transmission_channels(tbk_model* m, int axis, int layers, const double* k, int64_t nk, int M, int64_t n_s, const double* V,
                                         const double* onsite, int64_t n_z, const double* z, int max_iterations, int32_t* iterations, double* T,
                                         double* channels) {
    return tbk_transmission_channels_slab(m, 0, axis, layers, k, nk, M, n_s, V, onsite, n_z, z, max_iterations, iterations, T, channels);
}

extern "C" int tbk_transmission_channels_timing(tbk_model* m, double* ms, int64_t* calls, int reset) {
    TBK_ARG(m != nullptr && ms != nullptr && calls != nullptr, "model / ms / calls is NULL");
    return tbk_timed_read(m, TIMED_TRANSMISSION_CHANNELS, 3, ms, calls, nullptr, reset);
}
