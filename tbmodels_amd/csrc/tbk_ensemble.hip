// tbk_ensemble.hip -- the Landauer transmission of an ensemble of devices between the same two leads: disorder samples after one
// decimation (tools/ensemble_model.py).  T[k][z][s] is tbk_transmission's T of the device V_s, unchanged down to
// the order of the operations; the decimation of a (kp, z) does not depend on V, so it is computed once for a group of samples and
// the sweep with its closing once per sample.
//
//   transmission_ensemble_kernel<NP, DIAG>   a work item is (kp, z, group of consecutive samples): surf_load and surf_iterate once,
//                            then per sample trans_start, trans_layer x M and trans_closing on the planes the decimation left --
//                            trans_closing keeps es, et, H01 and H01^H, trans_start rebuilds D_1 from et.  N <= 64.  DIAG: the devices
//                            are real on-site energies [n_s][M][n]; trans_v (tbk_surface.h) gives the energy on the diagonal and 0.0
//                            elsewhere inside the expressions of the matrix form, so the bits are those of the expanded diagonal.
//   tbk_trans_ens_lib_chunk  65 <= N <= 1024, and on request: tbk_surface.hip's library route, surf_lib_iterate once per lockstep
//                            batch and the sweep per sample.
//
// The rule that splits the samples into groups, and EnsFamily, which tbk_channels.hip shares: tbk_ensemble.h.

#include <type_traits>

#include "tbk_ensemble.h"

namespace {

constexpr const char* ENS_FAMILY = "the transmission of an ensemble";
constexpr const char* ENS_NEEDS = "the transmission";  // what the shared messages call either route
constexpr const char* ENS_SINGULAR = "z - D of a device layer, or z - e of the decimation,";

// H00, H01, z, n_z, n, max_it, ws: transmission_kernel's.  V: n_s devices, [m_layers][n][n] complex each or, DIAG, [m_layers][n]
// doubles.  Item w = (k n_z + energy index) groups + g; group g takes the samples [g spg, min(n_s, (g + 1) spg)), never an empty
// range.  T_out: [nkc][n_z][n_s]; iters: [nkc][n_z], written by the group that holds sample 0.  The status word takes the smallest
// (((point index * SURF_MAX_Z + energy index) * ENS_MAX_SAMPLES + sample) * 2 + reason): reason 0 a zero pivot or a non-finite element
// in the sweep of that sample (a singular decimation raises it for every sample, so sample 0 is named), reason 1 the cap of the
// decimation with sample 0.  Every branch is workgroup-uniform; no index depends on a value but through the pivot tables; plain
// vector stores, one owner per output; a workgroup reads only its own slot.
template <int NP, bool DIAG>
__global__ void __launch_bounds__(SurfGeom<NP>::THREADS)
    transmission_ensemble_kernel(const double2* __restrict__ H00, const double2* __restrict__ H01, const void* __restrict__ V, int m_layers, int n_s, int spg,
                                 int groups, const double2* __restrict__ z, int n_z, int n, int64_t items, int max_it, unsigned long long key0, double* ws,
                                 int32_t* __restrict__ iters, double* __restrict__ T_out, unsigned long long* __restrict__ flag) {
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
            if (bad) atomicMin(flag, (key + (unsigned long long)s) * 2ull);
        }
        if (status == 2 && g == 0 && tid == 0) atomicMin(flag, key * 2ull + 1ull);
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
// the slots of the workgroups' matrices at NP = 64 for any chunk of at most `chunk` points
size_t ens_workspace_bytes(const EnsShape& sh, int64_t chunk, int n_cu) {
    return sh.n > 32 ? (size_t)surf_grid(sh.n, chunk * sh.n_z * sh.n_s, n_cu) * TransGeom<64>::slot_doubles * sizeof(double) : 0;
}

template <int NP, bool DIAG>
int ens_launch_np(const EnsShape& sh, const EnsLaunch& a) {
    using Geo = SurfGeom<NP>;
    static tbk_flag_row done;  // of this instantiation's kernel
    const void* kernel = reinterpret_cast<const void*>(transmission_ensemble_kernel<NP, DIAG>);
    if (TransGeom<NP>::lds_bytes > SURF_LDS_DEFAULT) TBK_HIP(tbk_raise_lds_limit(kernel, (int)TransGeom<NP>::lds_bytes, done));
    int64_t spg = 0, groups = 0;
    TBK_CHECK(ens_sample_groups<NP>(kernel, sh, a, spg, groups));
    const int64_t items = a.nkc * sh.n_z * groups;
    hipLaunchKernelGGL((transmission_ensemble_kernel<NP, DIAG>), dim3((unsigned)surf_grid(sh.n, items, a.n_cu)), dim3(Geo::THREADS), TransGeom<NP>::lds_bytes,
                       a.s, a.d_H00, a.d_H01, a.d_V, sh.m_layers, (int)sh.n_s, (int)spg, (int)groups, a.d_z, (int)sh.n_z, sh.n, items, a.max_it, a.key0,
                       a.d_ws, a.d_it, a.d_T, a.d_flag);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

// The ensemble's transmission of the chunk's nkc points at every energy on the own kernel
int ens_launch(const EnsShape& sh, const EnsLaunch& a) {
    return surf_with_np(sh.n, [&](auto np) {
        return sh.diag ? ens_launch_np<decltype(np)::value, true>(sh, a) : ens_launch_np<decltype(np)::value, false>(sh, a);
    });
}

// what the entry points check of the devices; the samples are staged once per call
int ens_check_devices(const EnsRoute& route, const EnsShape& sh, const double* V, const double* onsite, const int32_t* iterations, const double* T,
                      const double* channels) {
    if (route.channels && sh.n > SURF_OWN_MAX) {
        tbk_set_error("invalid argument: a principal layer of %d rows: %s takes at most %d", sh.n, route.family, SURF_OWN_MAX);
        return TBK_ERR_ARGUMENT;
    }
    TBK_ARG(sh.m_layers >= 1 && sh.m_layers <= TRANS_MAX_LAYERS, "the device must have 1 to 4096 principal layers");
    TBK_ARG(sh.n_s >= 1 && sh.n_s <= ENS_MAX_SAMPLES, "n_s must be 1 to 4096");
    TBK_ARG((V != nullptr) != (onsite != nullptr), "exactly one of V and onsite must be given");
    if (sh.device_bytes() > TRANS_DEVICE_BUDGET) {
        tbk_set_error("invalid argument: %lld devices of %d layers of %d rows: they may take at most 256 MiB", (long long)sh.n_s, sh.m_layers, sh.n);
        return TBK_ERR_ARGUMENT;
    }
    TBK_ARG(iterations != nullptr && T != nullptr, "iterations / T is NULL");
    TBK_ARG(!route.channels || channels != nullptr, "channels is NULL");
    return TBK_OK;
}

// The two status words of a chunk as one in the kernel's keys: the decimation of the library route names sample 0.
unsigned long long ens_chunk_word(const EnsRoute& route, const unsigned long long* two) {
    unsigned long long word = two[0];
    if (two[1] != SURF_NO_FLAG) word = std::min(word, (two[1] >> 1) * (unsigned long long)ENS_MAX_SAMPLES * route.radix + (two[1] & 1ull));
    return word;
}

// the status word as an error: the first (point, energy, sample) of the call that failed
int ens_status_error(const EnsRoute& route, unsigned long long word, const double* z, int max_iterations) {
    if (word == SURF_NO_FLAG) return TBK_OK;
    const int reason = (int)(word % route.radix);
    unsigned long long key = word / route.radix;
    const long long sample = (long long)(key % (unsigned long long)ENS_MAX_SAMPLES);
    key /= (unsigned long long)ENS_MAX_SAMPLES;
    const long long point = (long long)(key / (unsigned long long)SURF_MAX_Z), zi = (long long)(key % (unsigned long long)SURF_MAX_Z);
    if (reason == 0) {
        tbk_set_error("Singular matrix: %s at k index %lld, energy %lld (z = %.17g%+.17gj) and sample %lld", ENS_SINGULAR, point, zi, z[2 * zi],
                      z[2 * zi + 1], sample);
        return TBK_ERR_SINGULAR;
    }
    if (reason == 2) {
        tbk_set_error("the channel iteration (the Jacobi sweeps of the transmission eigenvalues) did not converge at k index %lld, energy %lld "
                      "(z = %.17g%+.17gj) and sample %lld",
                      point, zi, z[2 * zi], z[2 * zi + 1], sample);
        return TBK_ERR_NO_CONVERGENCE;
    }
    tbk_set_error("the decimation did not converge in %d iterations at k index %lld and energy %lld (z = %.17g%+.17gj)", max_iterations, point, zi,
                  z[2 * zi], z[2 * zi + 1]);
    return TBK_ERR_NO_CONVERGENCE;
}

const EnsRoute ENS_ROUTE = {ens_launch, 2u, false, TIMED_TRANSMISSION_ENSEMBLE, ENS_FAMILY};

}  // namespace

EnsFamily::EnsFamily(const EnsRoute& route_, int M, int64_t n_s, const double* V_, const double* onsite_, int64_t n_z, int64_t sample_chunk_,
                     int32_t* iterations_, double* T_, double* channels_)
    : route(route_), V(V_), onsite(onsite_), sample_chunk(sample_chunk_), iterations(iterations_), T(T_), channels(channels_) {
    family = route.family;
    needs = ENS_NEEDS;
    timed = route.timed;
    // ((n_k SURF_MAX_Z + n_z) ENS_MAX_SAMPLES + n_s) 2 + 1 < 2^64 needs n_k < 2^39; 2^36 leaves room, radix 4 included)
    max_points = int64_t(1) << 36;
    base_counts = true;
    bad_n_k = "n_k must be 1 to 2^36 - 1";
    bad_nk = "nk must be 0 to 2^36 - 1";
    n_words = 2;
    v_what = "the devices of the ensemble";
    sh.m_layers = M;
    sh.n_z = n_z;
    sh.n_s = n_s;
    sh.diag = onsite != nullptr;
    sh.channels = route.channels;
}

int EnsFamily::check(int N) {
    sh.n = N;
    TBK_CHECK(ens_check_devices(route, sh, V, onsite, iterations, T, channels));
    h_V = sh.diag ? onsite : V;
    v_bytes = sh.device_bytes();
    return TBK_OK;
}

int EnsFamily::check_options() const {
    TBK_ARG(sample_chunk >= 0, "sample_chunk < 0");
    return TBK_OK;
}

size_t EnsFamily::workspace_bytes(bool library, int64_t chunk, int n_cu) const {
    return library ? tbk_trans_ens_lib_bytes(sh.n) : ens_workspace_bytes(sh, chunk, n_cu);
}

int EnsFamily::run_chunk(bool library, const LayeredChunk& c) const {
    double* d_T = reinterpret_cast<double*>(c.d_res);
    int32_t* d_it = reinterpret_cast<int32_t*>(c.d_res + sh.t_bytes(c.nkc));
    double* d_ch = sh.channels ? reinterpret_cast<double*>(c.d_res + sh.t_bytes(c.nkc) + sh.it_bytes(c.nkc)) : nullptr;
    unsigned long long* d_flag = reinterpret_cast<unsigned long long*>(c.d_res + sh.result_bytes(c.nkc));
    if (library)
        return tbk_trans_ens_lib_chunk(c.s, c.blas, c.d_ws, sh.n, sh.m_layers, sh.n_s, c.d_H00, c.d_H01, sh.diag ? nullptr : static_cast<const double2*>(c.d_V),
                                       sh.diag ? static_cast<const double*>(c.d_V) : nullptr, c.d_z, sh.n_z, c.nkc, c.max_it, c.k0, d_it, d_T, d_flag);
    const EnsLaunch a = {c.s, c.n_cu, c.d_H00, c.d_H01, c.d_V, c.d_z, c.nkc, sample_chunk, c.max_it, (unsigned long long)c.k0 * (unsigned long long)SURF_MAX_Z,
                         reinterpret_cast<double*>(c.d_ws), d_it, d_T, d_flag, d_ch};
    return route.launch(sh, a);
}

int EnsFamily::copy_out(const LayeredCopy& copy, const char* d_res, int64_t nkc, int64_t c0) const {
    const size_t items = (size_t)nkc * sh.n_z, first = (size_t)c0 * sh.n_z;
    TBK_HIP(copy(T + first * sh.n_s, d_res, items * sh.n_s * sizeof(double)));
    TBK_HIP(copy(iterations + first, d_res + sh.t_bytes(nkc), items * sizeof(int32_t)));
    if (sh.channels) TBK_HIP(copy(channels + first * sh.n_s * sh.n, d_res + sh.t_bytes(nkc) + sh.it_bytes(nkc), items * sh.n_s * sh.n * sizeof(double)));
    return TBK_OK;
}

unsigned long long EnsFamily::chunk_word(const unsigned long long* words) const { return ens_chunk_word(route, words); }

int EnsFamily::status_error(unsigned long long word, const double* z, int max_iterations) const {
    return ens_status_error(route, word, z, max_iterations);
}

extern "C" int tbk_transmission_ensemble_from_matrices(int device, int N, int64_t n_k, const double* H00, const double* H01, int M, int64_t n_s,
                                                       const double* V, const double* onsite, int64_t n_z, const double* z, int max_iterations,
                                                       int64_t k_chunk, int64_t sample_chunk, int32_t* iterations, double* T) {
    EnsFamily fam(ENS_ROUTE, M, n_s, V, onsite, n_z, sample_chunk, iterations, T, nullptr);
    return layered_from_matrices(fam, device, N, n_k, H00, H01, n_z, z, max_iterations, k_chunk);
}

// The whole call on one handle; k_base as in tbk_surface_green_slab.  ws_mesh_io holds the samples.
int tbk_transmission_ensemble_slab(tbk_model* m, int64_t k_base, int axis, int layers, const double* k, int64_t nk, int M_device, int64_t n_s,
                                   const double* V, const double* onsite, int64_t n_z, const double* z, int max_iterations, int32_t* iterations,
                                   double* T) {
    EnsFamily fam(ENS_ROUTE, M_device, n_s, V, onsite, n_z, 0, iterations, T, nullptr);
    return layered_slab(fam, m, k_base, axis, layers, k, nk, n_z, z, max_iterations);
}

extern "C" int tbk_transmission_ensemble(tbk_model* m, int axis, int layers, const double* k, int64_t nk, int M, int64_t n_s, const double* V,
                                         const double* onsite, int64_t n_z, const double* z, int max_iterations, int32_t* iterations, double* T) {
    return tbk_transmission_ensemble_slab(m, 0, axis, layers, k, nk, M, n_s, V, onsite, n_z, z, max_iterations, iterations, T);
}

extern "C" int tbk_transmission_ensemble_timing(tbk_model* m, double* ms, int64_t* calls, int reset) {
    TBK_ARG(m != nullptr && ms != nullptr && calls != nullptr, "model / ms / calls is NULL");
    return tbk_timed_read(m, TIMED_TRANSMISSION_ENSEMBLE, 3, ms, calls, nullptr, reset);
}
