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
// The rule that splits the samples into groups, and the drivers tbk_channels.hip shares: tbk_ensemble.h.

#include <type_traits>

#include "tbk_ensemble.h"

namespace {

constexpr const char* ENS_FAMILY = "the transmission of an ensemble";
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
tbk_flag_row ens_lds_done[2][2];  // [NP = 32, 64][DIAG]: more than 64 KiB of dynamic LDS

// the slots of the workgroups' matrices at NP = 64 for any chunk of at most `chunk` points
size_t ens_workspace_bytes(const EnsShape& sh, int64_t chunk, int n_cu) {
    return sh.n > 32 ? (size_t)surf_grid(sh.n, chunk * sh.n_z * sh.n_s, n_cu) * TransGeom<64>::slot_doubles * sizeof(double) : 0;
}

template <int NP, bool DIAG>
int ens_launch_np(tbk_flag_row* done, const EnsShape& sh, const EnsLaunch& a) {
    using Geo = SurfGeom<NP>;
    const void* kernel = reinterpret_cast<const void*>(transmission_ensemble_kernel<NP, DIAG>);
    if (done != nullptr) TBK_HIP(tbk_raise_lds_limit(kernel, (int)TransGeom<NP>::lds_bytes, *done));
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
    if (sh.n <= 16) return sh.diag ? ens_launch_np<16, true>(nullptr, sh, a) : ens_launch_np<16, false>(nullptr, sh, a);
    if (sh.n <= 32) return sh.diag ? ens_launch_np<32, true>(&ens_lds_done[0][1], sh, a) : ens_launch_np<32, false>(&ens_lds_done[0][0], sh, a);
    return sh.diag ? ens_launch_np<64, true>(&ens_lds_done[1][1], sh, a) : ens_launch_np<64, false>(&ens_lds_done[1][0], sh, a);
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

// The kernel of `route` alone on principal layers the caller brings (tbk_transmission_ensemble_from_matrices and
// tbk_transmission_channels_from_matrices)
int tbk_ens_from_matrices(const EnsRoute& route, int device, int N, int64_t n_k, const double* H00, const double* H01, int M, int64_t n_s, const double* V,
                          const double* onsite, int64_t n_z, const double* z, int max_iterations, int64_t k_chunk, int64_t sample_chunk,
                          int32_t* iterations, double* T, double* channels) {
    TBK_CHECK(surf_check_energies(N, n_z, z, max_iterations));
    TBK_ARG(H01 != nullptr, "H01 is NULL: the transmission needs hopping between the principal layers");
    EnsShape sh;
    sh.n = N;
    sh.m_layers = M;
    sh.n_z = n_z;
    sh.n_s = n_s;
    sh.diag = onsite != nullptr;
    sh.channels = route.channels;
    TBK_CHECK(ens_check_devices(route, sh, V, onsite, iterations, T, channels));
    // ((n_k SURF_MAX_Z + n_z) ENS_MAX_SAMPLES + n_s) 2 + 1 < 2^64 needs n_k < 2^39; 2^36 leaves room, radix 4 included)
    TBK_ARG(n_k >= 1 && n_k < (int64_t(1) << 36), "n_k must be 1 to 2^36 - 1");
    TBK_ARG(H00 != nullptr, "H00 is NULL");
    TBK_ARG(k_chunk >= 0, "k_chunk < 0");
    TBK_ARG(sample_chunk >= 0, "sample_chunk < 0");
    TBK_CHECK(tetra_check_device(device));
    const int64_t chunk = std::min<int64_t>(n_k, k_chunk > 0 ? k_chunk : sh.auto_chunk(n_k));
    const int n_cu = surf_device_cus(device);
    const size_t nn = (size_t)N * N, h_bytes = (size_t)chunk * nn * sizeof(double2);
    DevBuf d_H00, d_H01, d_V, d_z, d_res, d_ws;
    TBK_CHECK(d_H00.reserve(h_bytes));
    TBK_CHECK(d_H01.reserve(h_bytes));
    TBK_CHECK(d_V.reserve(sh.device_bytes()));
    TBK_CHECK(d_z.reserve((size_t)n_z * sizeof(double2)));
    TBK_CHECK(d_res.reserve(sh.result_bytes(chunk) + EnsShape::flag_bytes));
    const bool library = N > SURF_OWN_MAX;  // (never with channels: ens_check_devices)
    const size_t ws_bytes = library ? tbk_trans_ens_lib_bytes(N) : ens_workspace_bytes(sh, chunk, n_cu);
    if (ws_bytes > 0) TBK_CHECK(d_ws.reserve(ws_bytes));
    Owned<rocblas_handle, rocblas_destroy_handle> blas;
    if (library) TBK_ROCBLAS(rocblas_create_handle(blas.put()));
    TBK_HIP(hipMemcpy(d_z.ptr, z, (size_t)n_z * sizeof(double2), hipMemcpyHostToDevice));
    TBK_HIP(hipMemcpy(d_V.ptr, sh.diag ? onsite : V, sh.device_bytes(), hipMemcpyHostToDevice));
    unsigned long long word = SURF_NO_FLAG;
    for (int64_t c0 = 0; c0 < n_k; c0 += chunk) {
        const int64_t nkc = std::min(chunk, n_k - c0);
        const size_t items = (size_t)nkc * n_z;
        char* res = d_res.as<char>();
        double* d_T = reinterpret_cast<double*>(res);
        int32_t* d_it = reinterpret_cast<int32_t*>(res + sh.t_bytes(nkc));
        double* d_ch = sh.channels ? reinterpret_cast<double*>(res + sh.t_bytes(nkc) + sh.it_bytes(nkc)) : nullptr;
        unsigned long long* d_flag = reinterpret_cast<unsigned long long*>(res + sh.result_bytes(nkc));
        TBK_HIP(hipMemcpy(d_H00.ptr, H00 + (size_t)c0 * nn * 2, (size_t)nkc * nn * sizeof(double2), hipMemcpyHostToDevice));
        TBK_HIP(hipMemcpy(d_H01.ptr, H01 + (size_t)c0 * nn * 2, (size_t)nkc * nn * sizeof(double2), hipMemcpyHostToDevice));
        TBK_HIP(hipMemset(d_flag, 0xff, EnsShape::flag_bytes));
        if (library) {
            TBK_CHECK(tbk_trans_ens_lib_chunk(nullptr, blas, d_ws.as<char>(), N, M, n_s, d_H00.as<double2>(), d_H01.as<double2>(),
                                              sh.diag ? nullptr : d_V.as<double2>(), sh.diag ? d_V.as<double>() : nullptr, d_z.as<double2>(), n_z, nkc,
                                              max_iterations, c0, d_it, d_T, d_flag));
        } else {
            const EnsLaunch a = {nullptr, n_cu, d_H00.as<double2>(), d_H01.as<double2>(), d_V.ptr, d_z.as<double2>(), nkc, sample_chunk, max_iterations,
                                 (unsigned long long)c0 * (unsigned long long)SURF_MAX_Z, d_ws.as<double>(), d_it, d_T, d_flag, d_ch};
            TBK_CHECK(route.launch(sh, a));
        }
        unsigned long long two[2] = {SURF_NO_FLAG, SURF_NO_FLAG};
        TBK_HIP(hipMemcpy(T + (size_t)c0 * n_z * n_s, d_T, items * n_s * sizeof(double), hipMemcpyDeviceToHost));
        TBK_HIP(hipMemcpy(iterations + (size_t)c0 * n_z, d_it, items * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (sh.channels) TBK_HIP(hipMemcpy(channels + (size_t)c0 * n_z * n_s * N, d_ch, items * n_s * N * sizeof(double), hipMemcpyDeviceToHost));
        TBK_HIP(hipMemcpy(two, d_flag, EnsShape::flag_bytes, hipMemcpyDeviceToHost));
        word = std::min(word, ens_chunk_word(route, two));
    }
    return ens_status_error(route, word, z, max_iterations);
}

extern "C" int tbk_transmission_ensemble_from_matrices(int device, int N, int64_t n_k, const double* H00, const double* H01, int M, int64_t n_s,
                                                       const double* V, const double* onsite, int64_t n_z, const double* z, int max_iterations,
                                                       int64_t k_chunk, int64_t sample_chunk, int32_t* iterations, double* T) {
    return tbk_ens_from_matrices(ENS_ROUTE, device, N, n_k, H00, H01, M, n_s, V, onsite, n_z, z, max_iterations, k_chunk, sample_chunk, iterations, T,
                                 nullptr);
}

// The whole call on one handle; k_base as in tbk_surface_green_slab.  The buffers are tbk_transmission's (tbk_internal.h), ws_mesh_io
// holding the samples.
int tbk_ens_slab(const EnsRoute& route, tbk_model* m, int64_t k_base, int axis, int layers, const double* k, int64_t nk, int M_device, int64_t n_s,
                 const double* V, const double* onsite, int64_t n_z, const double* z, int max_iterations, int32_t* iterations, double* T,
                 double* channels) {
    TBK_ARG(m != nullptr, "model is NULL");
    TBK_LOCK(m);
    TBK_ARG(!m->kdotp, "the transmission needs a tight-binding model");
    const int dim = m->dim, n_orb = m->n_orb;
    TBK_ARG(axis >= 0 && axis < dim, "axis must be 0 ... dim - 1");
    TBK_ARG(layers >= 1 && layers <= 1024, "layers must be 1 ... 1024: the transmission needs hopping along the axis");
    const int L = layers, M = 2 * L + 1;
    for (size_t r = 0; r < m->h_R.size() / (size_t)dim; ++r) {
        const int64_t reach = std::abs((int64_t)m->h_R[r * dim + axis]);
        if (reach > L) {
            tbk_set_error("invalid argument: layers = %d, but a stored hopping vector reaches %lld cells along axis %d", L, (long long)reach, axis);
            return TBK_ERR_ARGUMENT;
        }
    }
    const int64_t N64 = (int64_t)n_orb * L;
    TBK_CHECK(surf_check_energies((int)std::min<int64_t>(N64, 1 << 20), n_z, z, max_iterations));
    EnsShape sh;
    sh.n = (int)N64;
    sh.m_layers = M_device;
    sh.n_z = n_z;
    sh.n_s = n_s;
    sh.diag = onsite != nullptr;
    sh.channels = route.channels;
    const int N = sh.n;
    TBK_CHECK(ens_check_devices(route, sh, V, onsite, iterations, T, channels));
    TBK_ARG(nk >= 0 && k_base >= 0 && k_base + nk < (int64_t(1) << 36), "nk must be 0 to 2^36 - 1");
    if (nk == 0) return TBK_OK;
    TBK_ARG(k != nullptr || dim == 1, "k is NULL");
    const size_t nn2 = (size_t)n_orb * n_orb * 2;  // doubles of one H(k)
    const int64_t by_h = std::max<int64_t>(1, (int64_t)(SURF_CHUNK_BUDGET / ((size_t)M * nn2 * sizeof(double))));
    const int64_t chunk = std::min<int64_t>(nk, m->k_chunk > 0 ? m->k_chunk : std::min(sh.auto_chunk(nk), by_h));
    // (the host buffers the enqueued copies read and write, in front of the streams: they wait before these go)
    std::vector<double> h_k, h_tw;
    std::vector<unsigned long long> words;
    TBK_CHECK(surf_host_lists(dim, axis, L, k, nk, h_k, h_tw));
    try {
        words.assign((size_t)((nk + chunk - 1) / chunk) * 2, SURF_NO_FLAG);
    } catch (...) {
        tbk_set_error("cannot allocate the status words");
        return TBK_ERR_MEMORY;
    }
    MeshStreams streams;
    TBK_CHECK(streams.add(m));
    SpanRecorder* ev = &streams.used.back().ev;
    const size_t z_bytes = surf_align256((size_t)n_z * sizeof(double2)), tw_bytes = h_tw.size() * sizeof(double);
    const size_t layer_bytes = surf_align256((size_t)chunk * N * N * sizeof(double2));
    const bool library = !route.channels && (N > SURF_OWN_MAX || m->eigensolver == TBK_EIG_ROCSOLVER);  // (channels: the own kernel only)
    const size_t ws_bytes = library ? tbk_trans_ens_lib_bytes(N) : ens_workspace_bytes(sh, chunk, m->n_cu);
    TBK_CHECK(mesh_reserve(m->ws_mesh_k, h_k.size() * sizeof(double), route.family, "the k list with its samples along the stacking axis"));
    TBK_CHECK(mesh_reserve(m->ws_dm_r, z_bytes + tw_bytes, route.family, "the energies and the twiddles"));
    TBK_CHECK(mesh_reserve(m->ws_dm_rho, sh.result_bytes(chunk) + EnsShape::flag_bytes, route.family, "the results of one chunk"));
    TBK_CHECK(mesh_reserve(m->ws_dm_p, 2 * layer_bytes, route.family, "the principal layers of one chunk"));
    TBK_CHECK(mesh_reserve(m->ws_pdos_u, (size_t)chunk * M * nn2 * sizeof(double), route.family, "H(k) of one chunk"));
    TBK_CHECK(mesh_reserve(m->ws_mesh_io, sh.device_bytes(), route.family, "the devices of the ensemble"));
    if (ws_bytes > 0) TBK_CHECK(mesh_reserve(m->ws_mesh_work, ws_bytes, route.family, library ? "the library's batch" : "the workgroups' matrices"));
    if (library) m->counters[TBK_CNT_LIBRARY_CALLS] += 1;
    double* d_k = m->ws_mesh_k.as<double>();
    char* d_zt = m->ws_dm_r.as<char>();
    double* d_H = m->ws_pdos_u.as<double>();
    double2* d_H00 = m->ws_dm_p.as<double2>();
    double2* d_H01 = reinterpret_cast<double2*>(m->ws_dm_p.as<char>() + layer_bytes);
    const double2* d_z = reinterpret_cast<const double2*>(d_zt);
    char* d_res = m->ws_dm_rho.as<char>();
    TBK_HIP(hipMemcpyAsync(d_k, h_k.data(), h_k.size() * sizeof(double), hipMemcpyHostToDevice, m->stream));
    TBK_HIP(hipMemcpyAsync(d_zt, z, (size_t)n_z * sizeof(double2), hipMemcpyHostToDevice, m->stream));
    TBK_HIP(hipMemcpyAsync(d_zt + z_bytes, h_tw.data(), tw_bytes, hipMemcpyHostToDevice, m->stream));
    TBK_HIP(hipMemcpyAsync(m->ws_mesh_io.ptr, sh.diag ? onsite : V, sh.device_bytes(), hipMemcpyHostToDevice, m->stream));  // once per call
    for (int64_t c0 = 0, ci = 0; c0 < nk; c0 += chunk, ++ci) {
        const int64_t nkc = std::min(chunk, nk - c0);
        const size_t items = (size_t)nkc * n_z;
        double* d_T = reinterpret_cast<double*>(d_res);
        int32_t* d_it = reinterpret_cast<int32_t*>(d_res + sh.t_bytes(nkc));
        double* d_ch = sh.channels ? reinterpret_cast<double*>(d_res + sh.t_bytes(nkc) + sh.it_bytes(nkc)) : nullptr;
        unsigned long long* d_flag = reinterpret_cast<unsigned long long*>(d_res + sh.result_bytes(nkc));
        TBK_CHECK(surf_chunk_layers(m, ev, d_k + (size_t)c0 * M * dim, nkc, L, d_H, reinterpret_cast<const double*>(d_zt + z_bytes), d_H00, d_H01));
        TBK_HIP(hipMemsetAsync(d_flag, 0xff, EnsShape::flag_bytes, m->stream));
        if (ev) ev->start(1);
        if (library) {
            TBK_CHECK(tbk_trans_ens_lib_chunk(m->stream, m->blas, m->ws_mesh_work.as<char>(), N, M_device, n_s, d_H00, d_H01,
                                              sh.diag ? nullptr : m->ws_mesh_io.as<double2>(), sh.diag ? m->ws_mesh_io.as<double>() : nullptr, d_z, n_z,
                                              nkc, max_iterations, k_base + c0, d_it, d_T, d_flag));
        } else {
            const EnsLaunch a = {m->stream, m->n_cu, d_H00, d_H01, m->ws_mesh_io.ptr, d_z, nkc, 0, max_iterations,
                                 (unsigned long long)(k_base + c0) * (unsigned long long)SURF_MAX_Z, m->ws_mesh_work.as<double>(), d_it, d_T, d_flag, d_ch};
            TBK_CHECK(route.launch(sh, a));
        }
        if (ev) ev->stop();
        if (ev) ev->start(2);
        TBK_HIP(hipMemcpyAsync(T + (size_t)c0 * n_z * n_s, d_T, items * n_s * sizeof(double), hipMemcpyDeviceToHost, m->stream));
        TBK_HIP(hipMemcpyAsync(iterations + (size_t)c0 * n_z, d_it, items * sizeof(int32_t), hipMemcpyDeviceToHost, m->stream));
        if (sh.channels)
            TBK_HIP(hipMemcpyAsync(channels + (size_t)c0 * n_z * n_s * N, d_ch, items * n_s * N * sizeof(double), hipMemcpyDeviceToHost, m->stream));
        TBK_HIP(hipMemcpyAsync(&words[(size_t)ci * 2], d_flag, EnsShape::flag_bytes, hipMemcpyDeviceToHost, m->stream));
        if (ev) ev->stop();
    }
    TBK_CHECK(streams.finish((TimedFamily)route.timed));
    unsigned long long word = SURF_NO_FLAG;
    for (size_t ci = 0; ci < words.size(); ci += 2) word = std::min(word, ens_chunk_word(route, &words[ci]));
    return ens_status_error(route, word, z, max_iterations);
}

int tbk_transmission_ensemble_slab(tbk_model* m, int64_t k_base, int axis, int layers, const double* k, int64_t nk, int M_device, int64_t n_s,
                                   const double* V, const double* onsite, int64_t n_z, const double* z, int max_iterations, int32_t* iterations,
                                   double* T) {
    return tbk_ens_slab(ENS_ROUTE, m, k_base, axis, layers, k, nk, M_device, n_s, V, onsite, n_z, z, max_iterations, iterations, T, nullptr);
}

extern "C" int tbk_transmission_ensemble(tbk_model* m, int axis, int layers, const double* k, int64_t nk, int M, int64_t n_s, const double* V,
                                         const double* onsite, int64_t n_z, const double* z, int max_iterations, int32_t* iterations, double* T) {
    return tbk_transmission_ensemble_slab(m, 0, axis, layers, k, nk, M, n_s, V, onsite, n_z, z, max_iterations, iterations, T);
}

extern "C" int tbk_transmission_ensemble_timing(tbk_model* m, double* ms, int64_t* calls, int reset) {
    TBK_ARG(m != nullptr && ms != nullptr && calls != nullptr, "model / ms / calls is NULL");
    return tbk_timed_read(m, TIMED_TRANSMISSION_ENSEMBLE, 3, ms, calls, nullptr, reset);
}
