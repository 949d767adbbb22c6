// tbk_layered.hip -- the two host drivers of the calls on the stacked-layer geometry (tbk_layered.h), the principal
// layers of a chunk (surface_layers_kernel on the full H(k) of the handle's pipeline) and the checks and messages the families share.
// No line here knows a family: what differs between them comes through LayeredFamily.

#include "tbk_layered.h"

namespace {

// Hs: [n_k][2 L + 1][n][n], the full H(k) at k_a = j / (2 L + 1); tw: [2 L + 1][2 L + 1][2] (cos, sin) of -2 pi ((m j) mod (2 L + 1)) /
// (2 L + 1), row m + L.  One workgroup per in-plane point writes H00 and, L > 0, H01 [N][N], N = n max(L, 1): block (p, q) of H00 is
// H_{q-p}, of H01 H_{L+q-p} for q <= p and zero above.  H_m = (sum_j tw[m][j] Hs[j]) / (2 L + 1), j ascending.
__global__ void __launch_bounds__(256) surface_layers_kernel(const double2* __restrict__ Hs, const double* __restrict__ tw, int n, int L,
                                                             double2* __restrict__ H00, double2* __restrict__ H01) {
    const int M = 2 * L + 1, N = n * (L > 0 ? L : 1);
    const double2* hs = Hs + (size_t)blockIdx.x * M * n * n;
    double2* o0 = H00 + (size_t)blockIdx.x * N * N;
    double2* o1 = L > 0 ? H01 + (size_t)blockIdx.x * N * N : nullptr;
    for (int e = (int)threadIdx.x; e < N * N; e += 256) {
        const int I = e / N, J = e - I * N;
        const int p = I / n, i = I - p * n, q = J / n, j = J - q * n;
        for (int part = 0; part < (L > 0 ? 2 : 1); ++part) {
            const int m = part == 0 ? q - p : L + q - p;
            double sr = 0.0, si = 0.0;
            if (part == 0 || q <= p) {
                for (int s = 0; s < M; ++s) {
                    const double c = tw[((size_t)(m + L) * M + s) * 2], d = tw[((size_t)(m + L) * M + s) * 2 + 1];
                    const double2 h = hs[((size_t)s * n + i) * n + j];
                    sr += c * h.x - d * h.y;
                    si += c * h.y + d * h.x;
                }
                sr /= (double)M;
                si /= (double)M;
            }
            (part == 0 ? o0 : o1)[e] = make_double2(sr, si);
        }
    }
}

int surf_device_cus(int device) {
    int n_cu = 0;
    if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || n_cu < 1) n_cu = 256;
    return n_cu;
}

// The host lists of a whole call: per in-plane point the 2 L + 1 full k-points (k_a = j / (2 L + 1) inserted at `axis`), and the
// twiddles of surface_layers_kernel.
int surf_host_lists(int dim, int axis, int L, const double* k, int64_t nk, std::vector<double>& h_k, std::vector<double>& h_tw) {
    const int M = 2 * L + 1;
    try {
        h_k.resize((size_t)nk * M * dim);
        h_tw.resize((size_t)M * M * 2);
    } catch (...) {
        tbk_set_error("cannot allocate the k list");
        return TBK_ERR_MEMORY;
    }
    for (int64_t i = 0; i < nk; ++i)
        for (int j = 0; j < M; ++j) {
            double* dst = &h_k[((size_t)i * M + j) * dim];
            for (int d = 0, s = 0; d < dim; ++d) dst[d] = d == axis ? (double)j / (double)M : k[(size_t)i * (dim - 1) + s++];
        }
    const double two_pi = 6.283185307179586476925286766559;
    for (int mm = -L; mm <= L; ++mm)
        for (int j = 0; j < M; ++j) {
            const int num = ((mm * j) % M + M) % M;
            const double angle = -two_pi * (double)num / (double)M;
            h_tw[((size_t)(mm + L) * M + j) * 2] = std::cos(angle);
            h_tw[((size_t)(mm + L) * M + j) * 2 + 1] = std::sin(angle);
        }
    return TBK_OK;
}

// The chunk's principal layers: the FULL H(k) of its samples (d_k: the chunk's first), by the routine tbk_eigh_device uses, in pieces
// of its own choice, then surface_layers_kernel.  Stage 0 of the call's timer.
int surf_chunk_layers(tbk_model* m, SpanRecorder* ev, const double* d_k, int64_t nkc, int L, double* d_H, const double* d_tw, double2* d_H00,
                      double2* d_H01) {
    const int dim = m->dim, n_orb = m->n_orb, M = 2 * L + 1;
    const size_t nn2 = (size_t)n_orb * n_orb * 2;
    const int64_t npts = nkc * M;
    if (ev) ev->start(0);
    const int64_t piece = choose_chunk(m, npts, false);
    for (int64_t p0 = 0; p0 < npts; p0 += piece) {
        const int64_t np = std::min(piece, npts - p0);
        const tbk_hk_plan_t plan = tbk_hk_plan(m, tbk_staged_operand(m), np, false);
        TBK_CHECK(chunk_h(m, plan, HK_FULL, 2, d_k + (size_t)p0 * dim, nullptr, tbk_one_k_t(), d_H + (size_t)p0 * nn2));
    }
    hipLaunchKernelGGL(surface_layers_kernel, dim3((unsigned)nkc), dim3(256), 0, m->stream, reinterpret_cast<const double2*>(d_H), d_tw, n_orb, L, d_H00,
                       d_H01);
    TBK_HIP(hipGetLastError());
    if (ev) ev->stop();
    return TBK_OK;
}

}  // namespace

int surf_check_energies(int N, int64_t n_z, const double* z, int max_iterations) {
    TBK_ARG(N >= 1, "a principal layer has no rows");
    if (N > SURF_LIB_MAX) {
        tbk_set_error("invalid argument: a principal layer of %d rows: the decimation takes at most %d", N, SURF_LIB_MAX);
        return TBK_ERR_ARGUMENT;
    }
    TBK_ARG(n_z >= 1 && n_z <= SURF_MAX_Z, "n_z must be 1 to 4096");
    TBK_ARG(z != nullptr, "z is NULL");
    for (int64_t i = 0; i < n_z; ++i) {
        TBK_ARG(std::isfinite(z[2 * i]) && std::isfinite(z[2 * i + 1]), "an energy z is not finite");
        TBK_ARG(z[2 * i + 1] != 0.0, "every z needs Im z != 0");
    }
    TBK_ARG(max_iterations >= 1 && max_iterations <= SURF_MAX_ITERATIONS, "max_iterations must be 1 to 4096");
    return TBK_OK;
}

int trans_check_device(int N, int M, const double* V, const int32_t* iterations, const double* T) {
    TBK_ARG(M >= 1 && M <= TRANS_MAX_LAYERS, "the device must have 1 to 4096 principal layers");
    if ((size_t)M * N * N * sizeof(double2) > TRANS_DEVICE_BUDGET) {
        tbk_set_error("invalid argument: a device of %d layers of %d rows: V may take at most 256 MiB", M, N);
        return TBK_ERR_ARGUMENT;
    }
    TBK_ARG(V != nullptr, "V is NULL");
    TBK_ARG(iterations != nullptr && T != nullptr, "iterations / T is NULL");
    return TBK_OK;
}

int surf_status_error(unsigned long long word, const double* z, int max_iterations, const char* what) {
    if (word == SURF_NO_FLAG) return TBK_OK;
    const int reason = (int)(word & 1ull);
    const unsigned long long key = word >> 1;
    const long long point = (long long)(key / (unsigned long long)SURF_MAX_Z), zi = (long long)(key % (unsigned long long)SURF_MAX_Z);
    if (reason == 0) {
        tbk_set_error("Singular matrix: %s at k index %lld and energy %lld (z = %.17g%+.17gj)", what, point, zi, z[2 * zi], z[2 * zi + 1]);
        return TBK_ERR_SINGULAR;
    }
    tbk_set_error("the decimation did not converge in %d iterations at k index %lld and energy %lld (z = %.17g%+.17gj)", max_iterations, point, zi,
                  z[2 * zi], z[2 * zi + 1]);
    return TBK_ERR_NO_CONVERGENCE;
}

int layered_from_matrices(LayeredFamily& fam, int device, int N, int64_t n_k, const double* H00, const double* H01, int64_t n_z, const double* z,
                          int max_iterations, int64_t k_chunk) {
    // (every check of the arguments stands in front of the device's: none of them needs a GPU)
    TBK_CHECK(surf_check_energies(std::min(N, fam.rows_clamp), n_z, z, max_iterations));
    if (fam.min_layers > 0 && H01 == nullptr) {
        tbk_set_error("invalid argument: H01 is NULL: %s needs hopping between the principal layers", fam.needs);
        return TBK_ERR_ARGUMENT;
    }
    TBK_CHECK(fam.check(N));
    TBK_ARG(n_k >= 1 && n_k < fam.max_points, fam.bad_n_k);
    TBK_ARG(H00 != nullptr, "H00 is NULL");
    TBK_ARG(k_chunk >= 0, "k_chunk < 0");
    TBK_CHECK(fam.check_options());
    TBK_CHECK(tetra_check_device(device));
    const int64_t chunk = std::min<int64_t>(n_k, k_chunk > 0 ? k_chunk : fam.auto_chunk(n_k));
    const int n_cu = surf_device_cus(device);
    const size_t nn = (size_t)N * N, h_bytes = (size_t)chunk * nn * sizeof(double2), flag_bytes = (size_t)fam.n_words * sizeof(unsigned long long);
    DevBuf d_H00, d_H01, d_V, d_z, d_res, d_extra, d_ws;
    TBK_CHECK(d_H00.reserve(h_bytes));
    if (H01 != nullptr) TBK_CHECK(d_H01.reserve(h_bytes));
    if (fam.h_V != nullptr) TBK_CHECK(d_V.reserve(fam.v_bytes));
    TBK_CHECK(d_z.reserve((size_t)n_z * sizeof(double2)));
    TBK_CHECK(d_res.reserve(fam.result_bytes(chunk) + flag_bytes));
    const size_t extra_bytes = fam.extra_bytes(chunk, n_cu);
    if (extra_bytes > 0) TBK_CHECK(d_extra.reserve(extra_bytes));
    const bool library = fam.library(TBK_EIG_AUTO);
    const size_t ws_bytes = fam.workspace_bytes(library, chunk, n_cu);
    if (ws_bytes > 0) TBK_CHECK(d_ws.reserve(ws_bytes));
    Owned<rocblas_handle, rocblas_destroy_handle> blas;
    if (library) TBK_ROCBLAS(rocblas_create_handle(blas.put()));
    TBK_HIP(hipMemcpy(d_z.ptr, z, (size_t)n_z * sizeof(double2), hipMemcpyHostToDevice));
    if (fam.h_V != nullptr) TBK_HIP(hipMemcpy(d_V.ptr, fam.h_V, fam.v_bytes, hipMemcpyHostToDevice));
    unsigned long long word = SURF_NO_FLAG;
    for (int64_t c0 = 0; c0 < n_k; c0 += chunk) {
        const int64_t nkc = std::min(chunk, n_k - c0);
        char* res = d_res.as<char>();
        TBK_HIP(hipMemcpy(d_H00.ptr, H00 + (size_t)c0 * nn * 2, (size_t)nkc * nn * sizeof(double2), hipMemcpyHostToDevice));
        if (H01 != nullptr) TBK_HIP(hipMemcpy(d_H01.ptr, H01 + (size_t)c0 * nn * 2, (size_t)nkc * nn * sizeof(double2), hipMemcpyHostToDevice));
        TBK_HIP(hipMemset(res + fam.result_bytes(nkc), 0xff, flag_bytes));
        const LayeredChunk c = {nullptr, n_cu, blas, d_H00.as<double2>(), H01 != nullptr ? d_H01.as<double2>() : nullptr, d_V.ptr, d_z.as<double2>(),
                                d_ws.as<char>(), d_extra.as<char>(), nkc, c0, max_iterations, res};
        TBK_CHECK(fam.run_chunk(library, c));
        unsigned long long words[2] = {SURF_NO_FLAG, SURF_NO_FLAG};
        const LayeredCopy copy = {nullptr, false};
        TBK_CHECK(fam.copy_out(copy, res, nkc, c0));
        TBK_HIP(copy(words, res + fam.result_bytes(nkc), flag_bytes));
        word = std::min(word, fam.chunk_word(words));
    }
    return fam.status_error(word, z, max_iterations);
}

// The buffers are the handle's (tbk_internal.h): ws_mesh_k the k list with its samples along the stacking axis, ws_dm_r energies and
// twiddles, ws_dm_rho the results of one chunk and its status words, ws_dm_p its principal layers, ws_pdos_u its H(k), ws_mesh_io the
// family's potential, ws_mesh_u its second buffer, ws_mesh_work the workspace of the route.
int layered_slab(LayeredFamily& fam, tbk_model* m, int64_t k_base, int axis, int layers, const double* k, int64_t nk, int64_t n_z, const double* z,
                 int max_iterations) {
    TBK_ARG(m != nullptr, "model is NULL");
    TBK_LOCK(m);
    if (m->kdotp) {
        tbk_set_error("invalid argument: %s needs a tight-binding model", fam.needs);
        return TBK_ERR_ARGUMENT;
    }
    const int dim = m->dim, n_orb = m->n_orb;
    TBK_ARG(axis >= 0 && axis < dim, "axis must be 0 ... dim - 1");
    if (layers < fam.min_layers || layers > 1024) {
        if (fam.min_layers == 0)
            tbk_set_error("invalid argument: layers must be 0 ... 1024");
        else
            tbk_set_error("invalid argument: layers must be 1 ... 1024: %s needs hopping along the axis", fam.needs);
        return TBK_ERR_ARGUMENT;
    }
    const int L = layers, M = 2 * L + 1;
    for (size_t r = 0; r < m->h_R.size() / (size_t)dim; ++r) {
        const int64_t reach = std::abs((int64_t)m->h_R[r * dim + axis]);
        if (reach > L) {
            tbk_set_error("invalid argument: layers = %d, but a stored hopping vector reaches %lld cells along axis %d", L, (long long)reach, axis);
            return TBK_ERR_ARGUMENT;
        }
    }
    const int N = (int)std::min<int64_t>((int64_t)n_orb * std::max(L, 1), 1 << 20);
    TBK_CHECK(surf_check_energies(std::min(N, fam.rows_clamp), n_z, z, max_iterations));
    TBK_CHECK(fam.check(N));
    TBK_ARG(nk >= 0 && (fam.base_counts ? k_base >= 0 && k_base + nk < fam.max_points : nk < fam.max_points), fam.bad_nk);
    if (nk == 0) return TBK_OK;
    TBK_ARG(k != nullptr || dim == 1, "k is NULL");
    const size_t nn2 = (size_t)n_orb * n_orb * 2;  // doubles of one H(k)
    // k-points per chunk: the option, else what keeps the chunk's results and its H(k) samples inside the budget
    const int64_t by_h = std::max<int64_t>(1, (int64_t)(SURF_CHUNK_BUDGET / ((size_t)M * nn2 * sizeof(double))));
    const int64_t chunk = std::min<int64_t>(nk, m->k_chunk > 0 ? m->k_chunk : std::min(fam.auto_chunk(nk), by_h));
    // The host buffers that enqueued copies read and write -- h_k, h_tw and the status words -- are declared IN FRONT of the streams,
    // which wait for the handle before they go (tbk_resident.h).  This is the one place where the layered calls keep that rule.
    std::vector<double> h_k, h_tw;
    std::vector<unsigned long long> words;
    TBK_CHECK(surf_host_lists(dim, axis, L, k, nk, h_k, h_tw));
    try {
        words.assign((size_t)((nk + chunk - 1) / chunk) * fam.n_words, SURF_NO_FLAG);
    } catch (...) {
        tbk_set_error("cannot allocate the status words");
        return TBK_ERR_MEMORY;
    }
    MeshStreams streams;
    TBK_CHECK(streams.add(m));
    SpanRecorder* ev = &streams.used.back().ev;
    const size_t z_bytes = dos_align256((size_t)n_z * sizeof(double2)), tw_bytes = h_tw.size() * sizeof(double);
    const size_t layer_bytes = dos_align256((size_t)chunk * N * N * sizeof(double2)), flag_bytes = (size_t)fam.n_words * sizeof(unsigned long long);
    const bool library = fam.library(m->eigensolver);
    const size_t extra_bytes = fam.extra_bytes(chunk, m->n_cu), ws_bytes = fam.workspace_bytes(library, chunk, m->n_cu);
    TBK_CHECK(mesh_reserve(m->ws_mesh_k, h_k.size() * sizeof(double), fam.family, "the k list with its samples along the stacking axis"));
    TBK_CHECK(mesh_reserve(m->ws_dm_r, z_bytes + tw_bytes, fam.family, "the energies and the twiddles"));
    TBK_CHECK(mesh_reserve(m->ws_dm_rho, fam.result_bytes(chunk) + flag_bytes, fam.family, "the results of one chunk"));
    TBK_CHECK(mesh_reserve(m->ws_dm_p, 2 * layer_bytes, fam.family, "the principal layers of one chunk"));
    TBK_CHECK(mesh_reserve(m->ws_pdos_u, (size_t)chunk * M * nn2 * sizeof(double), fam.family, "H(k) of one chunk"));
    if (fam.h_V != nullptr) TBK_CHECK(mesh_reserve(m->ws_mesh_io, fam.v_bytes, fam.family, fam.v_what));
    if (extra_bytes > 0) TBK_CHECK(mesh_reserve(m->ws_mesh_u, extra_bytes, fam.family, fam.extra_what));
    if (ws_bytes > 0) TBK_CHECK(mesh_reserve(m->ws_mesh_work, ws_bytes, fam.family, library ? "the library's batch" : "the workgroups' matrices"));
    if (library) m->counters[TBK_CNT_LIBRARY_CALLS] += 1;
    double* d_k = m->ws_mesh_k.as<double>();
    char* d_zt = m->ws_dm_r.as<char>();
    double* d_H = m->ws_pdos_u.as<double>();
    double2* d_H00 = m->ws_dm_p.as<double2>();
    double2* d_H01 = L > 0 ? reinterpret_cast<double2*>(m->ws_dm_p.as<char>() + layer_bytes) : nullptr;
    char* d_res = m->ws_dm_rho.as<char>();
    TBK_HIP(hipMemcpyAsync(d_k, h_k.data(), h_k.size() * sizeof(double), hipMemcpyHostToDevice, m->stream));
    TBK_HIP(hipMemcpyAsync(d_zt, z, (size_t)n_z * sizeof(double2), hipMemcpyHostToDevice, m->stream));
    TBK_HIP(hipMemcpyAsync(d_zt + z_bytes, h_tw.data(), tw_bytes, hipMemcpyHostToDevice, m->stream));
    if (fam.h_V != nullptr) TBK_HIP(hipMemcpyAsync(m->ws_mesh_io.ptr, fam.h_V, fam.v_bytes, hipMemcpyHostToDevice, m->stream));  // once per call
    const LayeredCopy copy = {m->stream, true};
    for (int64_t c0 = 0, ci = 0; c0 < nk; c0 += chunk, ++ci) {
        const int64_t nkc = std::min(chunk, nk - c0);
        TBK_CHECK(surf_chunk_layers(m, ev, d_k + (size_t)c0 * M * dim, nkc, L, d_H, reinterpret_cast<const double*>(d_zt + z_bytes), d_H00, d_H01));
        TBK_HIP(hipMemsetAsync(d_res + fam.result_bytes(nkc), 0xff, flag_bytes, m->stream));
        if (ev) ev->start(1);
        const LayeredChunk c = {m->stream, m->n_cu, m->blas, d_H00, d_H01, fam.h_V != nullptr ? m->ws_mesh_io.ptr.h : nullptr,
                                reinterpret_cast<const double2*>(d_zt), m->ws_mesh_work.as<char>(), m->ws_mesh_u.as<char>(), nkc, k_base + c0,
                                max_iterations, d_res};
        TBK_CHECK(fam.run_chunk(library, c));
        if (ev) ev->stop();
        if (ev) ev->start(2);
        TBK_CHECK(fam.copy_out(copy, d_res, nkc, c0));
        TBK_HIP(copy(&words[(size_t)ci * fam.n_words], d_res + fam.result_bytes(nkc), flag_bytes));
        if (ev) ev->stop();
    }
    // synchronises the handle and books the kernel times; then the status words, the smallest (point, energy) first
    TBK_CHECK(streams.finish(fam.timed));
    unsigned long long word = SURF_NO_FLAG;
    for (size_t at = 0; at < words.size(); at += fam.n_words) word = std::min(word, fam.chunk_word(&words[at]));
    return fam.status_error(word, z, max_iterations);
}
