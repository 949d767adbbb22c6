// tbk_lattice.hip -- the host drivers of the calls that Fourier-sum a matrix of a k mesh into lattice vectors (tbk_lattice.h,
// DESIGN.md 20.8) and the plan of their chunks and energy tiles.  No line here knows a family: what differs between them comes
// through LatticeFamily.

#include "tbk_lattice.h"

GreenPlan green_plan(const DmPlan& D, int64_t n_z, int64_t z_tile, int64_t k_chunk, int64_t auto_chunk) {
    GreenPlan G;
    G.D = D;
    G.n_z = n_z;
    G.bt = D.n <= 16 ? 1 : 4;
    const int64_t want = std::min<int64_t>(n_z, z_tile > 0 ? std::min<int64_t>(z_tile, GREEN_ZT) : GREEN_ZT);
    const size_t per_point = (size_t)D.n2 * sizeof(double2);  // of one energy
    if (k_chunk > 0) {
        G.chunk = dm_cap_chunk(D, std::min(k_chunk, D.rows));
        const int64_t by_budget = (int64_t)(GREEN_P_BUDGET / (per_point * (size_t)(D.groups(G.chunk) * 4)));
        G.zt = std::max<int64_t>(1, std::min(want, by_budget));
    } else {
        G.zt = want;
        const int64_t by_budget = (int64_t)(GREEN_P_BUDGET / (per_point * (size_t)want)) - 8;
        G.chunk = dm_cap_chunk(D, std::max<int64_t>(4, std::min(std::min(auto_chunk, D.rows), by_budget)));
    }
    G.tiles = (n_z + G.zt - 1) / G.zt;
    return G;
}

namespace {

// the constants of a call in one small buffer: the reduced lattice vectors and, each 256-byte aligned, the energies and the self-energy
struct LatticeConstants {
    size_t rm_bytes, z_off, z_bytes, s_off, s_bytes;
    LatticeConstants(const LatticeFamily& fam, const DmPlan& D)
        : rm_bytes((size_t)D.n_r * D.mesh.dim * sizeof(int32_t)), z_off(dos_align256(rm_bytes)), z_bytes(fam.z ? (size_t)fam.n_z * sizeof(double2) : 0),
          s_off(dos_align256(z_off + z_bytes)), s_bytes(fam.sigma ? (size_t)fam.n_z * D.n2 * sizeof(double2) : 0) {}
    size_t bytes() const { return s_bytes ? s_off + s_bytes : z_bytes ? z_off + z_bytes : rm_bytes; }
};

// the chunk's phase table once, then per tile of energies the family's P and its contraction into the tile's partials: stages 0, 1, 2
int lattice_chunk(const LatticeFamily& fam, const LatticeChunk& c, SpanRecorder* ev, const int32_t* d_Rm, double* d_tab, char* d_part) {
    const GreenPlan& G = c.G;
    TBK_CHECK(dm_launch_phase(c.s, G.D, ev, d_Rm, c.c0, c.nkc, d_tab));
    for (int64_t t = 0; t < G.tiles; ++t) {
        if (ev) ev->start(1);
        TBK_CHECK(fam.fill_p(c, t));
        if (ev) ev->stop();
        TBK_HIP(hipGetLastError());
        TBK_CHECK(dm_launch_fourier(c.s, G.tile_plan(t), ev, c.c0, c.nkc, d_tab, c.d_P, reinterpret_cast<double2*>(d_part + (size_t)t * G.part_stride())));
    }
    return TBK_OK;
}

// The slab's result in device memory.  gather: every tile's slices summed (the scratch of one tile behind G) and its block of
// energies put into G [n_r][n_z][n^2] at d_res; else the one tile's sum where dm_launch_reduce leaves it.
int lattice_result(hipStream_t s, const GreenPlan& G, SpanRecorder* ev, const char* d_part, char* d_res, const void** result) {
    const DmPlan& D = G.D;
    double2* d_sum = reinterpret_cast<double2*>(d_res + G.sum_offset());
    for (int64_t t = 0; t < G.tiles; ++t) {
        const int64_t zt = G.tile_count(t);
        const double2* d_tile = nullptr;
        TBK_CHECK(dm_launch_reduce(s, G.tile_plan(t), ev, reinterpret_cast<const double2*>(d_part + (size_t)t * G.part_stride()), d_sum, &d_tile));
        *result = d_tile;
        if (!G.gather) continue;
        const size_t width = (size_t)zt * D.n2 * sizeof(double2);
        TBK_HIP(hipMemcpy2DAsync(reinterpret_cast<double2*>(d_res) + (size_t)t * G.zt * D.n2, (size_t)G.n_z * D.n2 * sizeof(double2), d_tile, width, width,
                                 (size_t)D.n_r, hipMemcpyDeviceToDevice, s));
        *result = d_res;
    }
    return TBK_OK;
}

}  // namespace

int lattice_from_arrays(LatticeFamily& fam, int dim, const int32_t* mesh, int64_t nk, int n_orb, const double* E, const double* mat, int64_t k_chunk,
                        int64_t z_tile, int64_t n_r, const int64_t* R, double* out) {
    fam.dim = dim;
    fam.mesh = mesh;
    DmPlan D;
    TBK_CHECK(dm_plan(dim, mesh, nk, 0, nk, n_orb, n_r, &D));
    const GreenPlan G = fam.plan(D, z_tile, k_chunk, nk);
    std::vector<int32_t> h_Rm;
    TBK_CHECK(dm_reduce_R(dim, mesh, n_r, R, &h_Rm));
    const LatticeConstants C(fam, D);
    const bool library = fam.library(n_orb, TBK_EIG_AUTO);
    DevBuf d_in, d_const, d_tab, d_P, d_part, d_res, d_flag, d_work;
    Owned<rocblas_handle, rocblas_destroy_handle> blas;
    TBK_CHECK(d_part.reserve(G.part_bytes()));
    if (G.result_bytes() > 0) TBK_CHECK(d_res.reserve(G.result_bytes()));
    TBK_CHECK(d_const.reserve(C.bytes()));
    if (fam.has_status) TBK_CHECK(d_flag.reserve(sizeof(unsigned long long)));
    TBK_CHECK(d_in.reserve(G.in_bytes(fam.needs_h)));
    TBK_CHECK(d_tab.reserve(D.tab_bytes(G.chunk)));
    TBK_CHECK(d_P.reserve(G.p_bytes()));
    if (library) {
        TBK_CHECK(d_work.reserve(fam.work_bytes(G)));
        TBK_ROCBLAS(rocblas_create_handle(blas.put()));
    }
    char* d_c = d_const.as<char>();
    TBK_HIP(hipMemcpy(d_c, h_Rm.data(), C.rm_bytes, hipMemcpyHostToDevice));
    if (C.z_bytes) TBK_HIP(hipMemcpy(d_c + C.z_off, fam.z, C.z_bytes, hipMemcpyHostToDevice));
    if (C.s_bytes) TBK_HIP(hipMemcpy(d_c + C.s_off, fam.sigma, C.s_bytes, hipMemcpyHostToDevice));
    if (fam.has_status) TBK_HIP(hipMemset(d_flag.ptr, 0xff, sizeof(unsigned long long)));
    TBK_HIP(hipMemset(d_part.ptr, 0, G.part_bytes()));
    const size_t e_per_k = (size_t)n_orb, m_per_k = (size_t)D.n2 * 2;  // doubles
    for (int64_t c0 = 0; c0 < nk; c0 += G.chunk) {
        const int64_t nkc = std::min(G.chunk, nk - c0), pad = c0 & 3;
        const LatticeChunk c = {nullptr, G, c0, nkc, pad, (pad + nkc + 3) / 4, d_in.as<double>(), reinterpret_cast<const double2*>(d_c + C.z_off),
                                reinterpret_cast<const double2*>(d_c + C.s_off), d_flag.as<unsigned long long>(), blas, d_work.as<char>(), d_P.as<double2>()};
        // (the next chunk's upload overwrites the last one's: the null stream orders it behind the kernels)
        if (E != nullptr)
            TBK_HIP(hipMemcpy(c.d_E(), E + (size_t)c0 * e_per_k, (size_t)nkc * e_per_k * sizeof(double), hipMemcpyHostToDevice));
        TBK_HIP(hipMemcpy(d_in.ptr, mat + (size_t)c0 * m_per_k, (size_t)nkc * m_per_k * sizeof(double), hipMemcpyHostToDevice));
        TBK_CHECK(lattice_chunk(fam, c, nullptr, d_const.as<int32_t>(), d_tab.as<double>(), d_part.as<char>()));
    }
    const void* d_result = nullptr;
    TBK_CHECK(lattice_result(nullptr, G, nullptr, d_part.as<char>(), d_res.as<char>(), &d_result));
    if (fam.has_status) {
        unsigned long long word = GREEN_NO_FLAG;
        TBK_HIP(hipMemcpy(&word, d_flag.ptr, sizeof(word), hipMemcpyDeviceToHost));
        TBK_CHECK(fam.status_error(word));
    }
    TBK_HIP(hipMemcpy(out, d_result, G.g_bytes(), hipMemcpyDeviceToHost));
    return TBK_OK;
}

int LatticeCall::open(LatticeFamily& fam, const TetraHandles& th, const int32_t* mesh, int64_t n_r_, const int64_t* R, double* out_, size_t slabs) {
    fam.dim = th.dim;
    fam.mesh = mesh;
    n_r = n_r_;
    out = out_;
    out_doubles = (size_t)n_r * fam.n_z * th.n_orb * th.n_orb * 2;
    h_k.resize(slabs);
    partial.resize(slabs);
    words.assign(slabs, GREEN_NO_FLAG);
    return dm_reduce_R(th.dim, mesh, n_r, R, &h_Rm);
}

// (the buffers are the handle's: tbk_internal.h says which keeps what)
int lattice_slab(LatticeFamily& fam, const TetraHandles& th, LatticeCall& call, size_t slab, tbk_model* m, SpanRecorder* ev, const double* d_k,
                 int64_t nk, int64_t first_pt) {
    const int dim = th.dim, n_orb = th.n_orb;
    DmPlan D;
    TBK_CHECK(dm_plan(dim, fam.mesh, th.nk_total, first_pt, nk, n_orb, call.n_r, &D));
    // The result and its partials first (the tile does not depend on the automatic chunk): the chunk is chosen from the memory
    // they leave, shared between what the chunk's P is made from, the P of one tile and, on the library route, its batch.
    const bool library = fam.library(n_orb, m->eigensolver);
    const LatticeConstants C(fam, D);
    GreenPlan G = fam.plan(D, 0, m->k_chunk, nk);
    TBK_CHECK(mesh_reserve(m->ws_dm_part, G.part_bytes(), fam.family, fam.part_what));
    if (G.result_bytes() > 0) TBK_CHECK(mesh_reserve(m->ws_dm_rho, G.result_bytes(), fam.family, fam.result_what));
    TBK_CHECK(mesh_reserve(m->ws_dm_r, C.bytes(), fam.family, fam.const_what));
    if (fam.has_status) {
        TBK_CHECK(m->ws_green_flag.reserve(sizeof(unsigned long long)));
        TBK_HIP(hipMemsetAsync(m->ws_green_flag.ptr, 0xff, sizeof(unsigned long long), m->stream));  // (a call that ended early may have left it raised)
    }
    G = fam.plan(D, 0, m->k_chunk, mesh_eigh_chunk(m, nk, fam.share((int)G.zt, library)));
    TBK_CHECK(mesh_reserve(m->ws_pdos_u, G.in_bytes(fam.needs_h), fam.family, fam.in_what));
    TBK_CHECK(m->ws_dm_tab.reserve(D.tab_bytes(G.chunk)));
    TBK_CHECK(mesh_reserve(m->ws_dm_p, G.p_bytes(), fam.family, fam.p_what));
    if (library) {
        TBK_CHECK(mesh_reserve(m->ws_mesh_work, fam.work_bytes(G), fam.family, fam.work_what));
        m->counters[TBK_CNT_LIBRARY_CALLS] += 1;
    }
    char* d_c = m->ws_dm_r.as<char>();
    TBK_HIP(hipMemcpyAsync(d_c, call.h_Rm.data(), C.rm_bytes, hipMemcpyHostToDevice, m->stream));
    if (C.z_bytes) TBK_HIP(hipMemcpyAsync(d_c + C.z_off, fam.z, C.z_bytes, hipMemcpyHostToDevice, m->stream));
    if (C.s_bytes) TBK_HIP(hipMemcpyAsync(d_c + C.s_off, fam.sigma, C.s_bytes, hipMemcpyHostToDevice, m->stream));
    TBK_HIP(hipMemsetAsync(m->ws_dm_part.ptr, 0, G.part_bytes(), m->stream));
    double* d_in = m->ws_pdos_u.as<double>();
    const size_t nn2 = (size_t)D.n2 * 2;
    for (int64_t c0 = 0; c0 < nk; c0 += G.chunk) {
        const int64_t nkc = std::min(G.chunk, nk - c0), pad = c0 & 3;
        const LatticeChunk c = {m->stream, G, c0, nkc, pad, (pad + nkc + 3) / 4, d_in, reinterpret_cast<const double2*>(d_c + C.z_off),
                                reinterpret_cast<const double2*>(d_c + C.s_off), m->ws_green_flag.as<unsigned long long>(), library ? m->blas : nullptr,
                                m->ws_mesh_work.as<char>(), m->ws_dm_p.as<double2>()};
        if (fam.needs_h) {
            // the FULL H(k) of the chunk, by the routine tbk_eigh_device uses, in pieces of its own choice (the handle is locked)
            const int64_t piece = choose_chunk(m, nkc, false);
            for (int64_t p0 = 0; p0 < nkc; p0 += piece) {
                const int64_t np = std::min(piece, nkc - p0);
                const tbk_hk_plan_t plan = tbk_hk_plan(m, tbk_staged_operand(m), np, false);
                TBK_CHECK(chunk_h(m, plan, HK_FULL, 2, d_k + (c0 + p0) * dim, nullptr, tbk_one_k_t(), d_in + (size_t)p0 * nn2));
            }
        } else {
            // (a family that does not use the chunk's eigenvalues gets them behind its eigenvectors all the same)
            TBK_CHECK(tbk_eigh_device(m, d_k + c0 * dim, nkc, 2, nullptr, c.d_E(), d_in));
        }
        TBK_CHECK(lattice_chunk(fam, c, ev, reinterpret_cast<const int32_t*>(d_c), m->ws_dm_tab.as<double>(), m->ws_dm_part.as<char>()));
    }
    const void* d_result = nullptr;
    TBK_CHECK(lattice_result(m->stream, G, ev, m->ws_dm_part.as<char>(), m->ws_dm_rho.as<char>(), &d_result));
    double* h_dst = call.out;
    if (slab > 0) {
        try {
            call.partial[slab].resize(call.out_doubles);
        } catch (...) {
            tbk_set_error("cannot allocate the per-handle results");
            return TBK_ERR_MEMORY;
        }
        h_dst = call.partial[slab].data();
    }
    TBK_HIP(hipMemcpyAsync(h_dst, d_result, G.g_bytes(), hipMemcpyDeviceToHost, m->stream));
    if (fam.has_status) {
        // the status word comes down with the result and is cleared for the next call
        TBK_HIP(hipMemcpyAsync(&call.words[slab], m->ws_green_flag.ptr, sizeof(unsigned long long), hipMemcpyDeviceToHost, m->stream));
        TBK_HIP(hipMemsetAsync(m->ws_green_flag.ptr, 0xff, sizeof(unsigned long long), m->stream));
    }
    return TBK_OK;
}

int lattice_finish(const LatticeFamily& fam, LatticeCall& call, MeshStreams& streams) {
    TBK_CHECK(streams.finish(fam.timed));
    unsigned long long word = GREEN_NO_FLAG;
    for (unsigned long long w : call.words) word = std::min(word, w);
    TBK_CHECK(fam.status_error(word));
    for (size_t i = 1; i < call.partial.size(); ++i)  // in handle order
        for (size_t x = 0; x < call.out_doubles; ++x) call.out[x] += call.partial[i][x];
    return TBK_OK;
}
