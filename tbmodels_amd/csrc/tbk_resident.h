// tbk_resident.h -- what the mesh calls on staged handles share on the host once their kernels are enqueued, and the calls that keep
// the eigensystem of the WHOLE mesh resident on every busy handle and run their kernels on it: tbk_chi.hip (the three
// susceptibilities) and tbk_berry.hip (the Berry flux).  Two objects, no kernels:
//
//   MeshStreams   the busy handles of one call with their span recorders: the mid-call check, the finish, the wait on every exit.
//                 TetraStaged (tbk_tetra_staged.h: every tetrahedron call, and through OccStaged tbk_dm.hip) holds one, ResidentMesh
//                 holds one.
//   ResidentMesh  the k list of the mesh and, per handle, the steps in the order a caller takes them: stage (the reservations of
//                 k, E and U), the caller's own reservations, upload, the caller's own copies, fill, the caller's launches.
#pragma once

#include <algorithm>
#include <cmath>
#include <deque>
#include <vector>

#include "tbk_tetra.h"

// k-points per chunk of an eigenvector walk over nk points: TBK_OPT_K_CHUNK as given, else what the eigenvector call itself would
// take from the free memory, over `share` (the buffers a caller keeps beside the chunk's eigenvectors)
inline int64_t mesh_eigh_chunk(tbk_model* m, int64_t nk, int share = 1) {
    return std::max<int64_t>(1, std::min<int64_t>(nk, m->k_chunk > 0 ? m->k_chunk : choose_chunk(m, nk, true) / share));
}

// a reservation whose failure names the family ("the susceptibility"), what it keeps (NULL: the plain message) and the bytes
inline int mesh_reserve(DevBuf& buf, size_t bytes, const char* family, const char* what) {
    const int r = buf.reserve(bytes);
    if (r == TBK_ERR_MEMORY && what) tbk_set_error("%s keeps %s in device memory: %zu bytes do not fit", family, what, bytes);
    return r;
}

// D[n_q][n_orb] (re, im) of convention 1: exp(-2 pi i sum_d q_d pos[i][d] / n_d), the unreduced q_d (tools/chi_model.py phase_table)
inline int mesh_phase_table(int dim, const int32_t* mesh, int n_orb, int64_t n_q, const int64_t* q, const double* pos, std::vector<double>* out) {
    try {
        out->resize((size_t)n_q * n_orb * 2);
    } catch (...) {
        tbk_set_error("cannot allocate the orbital phases");
        return TBK_ERR_MEMORY;
    }
    const double two_pi = 6.283185307179586476925286766559;
    for (int64_t r = 0; r < n_q; ++r)
        for (int i = 0; i < n_orb; ++i) {
            double angle = 0.0;
            for (int d = 0; d < dim; ++d) angle = angle + ((double)q[r * dim + d] * pos[(size_t)i * dim + d]) / (double)mesh[d];
            angle = -two_pi * angle;
            (*out)[((size_t)r * n_orb + i) * 2] = std::cos(angle);
            (*out)[((size_t)r * n_orb + i) * 2 + 1] = std::sin(angle);
        }
    return TBK_OK;
}

// The busy handles of one mesh call, in handle order, each with the recorder of its kernel spans.  When the object goes it waits for
// what the call has enqueued on their streams, however the call ends: a copy into or out of a host buffer may be pending when an
// error of a later handle returns.  So every host buffer that an enqueued copy reads or writes and that the call owns is DECLARED IN
// FRONT of this object (or of the one that holds it), never behind it: what is declared behind is destroyed before the wait.
struct MeshStreams {
    struct Use {
        tbk_model* m;
        SpanRecorder ev;
    };
    std::deque<Use> used;  // (a deque: a recorder stays where it is while handles are added)
    ~MeshStreams() {
        for (Use& u : used)
            if (hipSetDevice(u.m->device) == hipSuccess) (void)hipStreamSynchronize(u.m->stream);
    }

    // the option check; the handle's device made current; from here on the exit waits for its stream
    int add(tbk_model* m) {
        TBK_CHECK(tbk_eig_check_option(m));
        TBK_HIP(hipSetDevice(m->device));
        used.push_back({m, SpanRecorder(m->timing, m->stream)});
        return TBK_OK;
    }

    // synchronises every handle; non-finite eigenvalues / no convergence end the call here, as in tbk_eigenval and tbk_eigh: the
    // first failing handle's
    int check() {
        for (Use& u : used) TBK_CHECK(tbk_eigenval_check(u.m));
        return TBK_OK;
    }

    // every handle waited for and its kernel times booked on the family's row: for a call that has enqueued no eigensystem since its
    // last check().  timed_only: the row counts the calls made under TBK_OPT_TIMING alone (dos, pdos)
    int book(TimedFamily family, bool timed_only = false) {
        for (Use& u : used) {
            TBK_HIP(hipSetDevice(u.m->device));
            TBK_HIP(hipStreamSynchronize(u.m->stream));
            u.ev.collect(u.m->timed[family].ms);
            if (u.ev.on || !timed_only) u.m->timed[family].calls += 1;
        }
        return TBK_OK;
    }

    // check, then book
    int finish(TimedFamily family) {
        TBK_CHECK(check());
        return book(family);
    }
};

// The eigensystem of the whole mesh on every busy handle: k in ws_mesh_k, E in ws_mesh_e, U in ws_mesh_u (tbk_internal.h).  The k
// list is the source of every handle's upload and the fold hint of its fill, so it lives here, in front of the streams.
struct ResidentMesh {
    int dim = 0, n_orb = 0;
    int64_t nk = 0;
    std::vector<double> h_k;  // [nk][dim] in mesh order
    MeshStreams streams;      // (behind h_k: it waits before h_k goes)

    int open(int dim_, const int32_t* mesh, int n_orb_, int64_t nk_) {
        dim = dim_;
        n_orb = n_orb_;
        nk = nk_;
        return tbk_dos_mesh_klist(dim, mesh, 0, mesh[0], &h_k);
    }

    // MeshStreams::add, then the reservations: k, E -- e_bytes of it, e_what the family's text for them (chi keeps E and two Fermi
    // tables, Berry E alone) -- and, with_u, U.  The caller makes all of its own reservations next, before fill: the eigensolver
    // sizes its chunk from the memory that is free then.
    int stage(tbk_model* m, const char* family, size_t e_bytes, const char* e_what, bool with_u) {
        TBK_CHECK(streams.add(m));
        TBK_CHECK(m->ws_mesh_k.reserve(h_k.size() * sizeof(double)));
        TBK_CHECK(mesh_reserve(m->ws_mesh_e, e_bytes, family, e_what));
        if (with_u)
            TBK_CHECK(mesh_reserve(m->ws_mesh_u, (size_t)nk * n_orb * n_orb * sizeof(double2), family, "the eigenvectors of the whole mesh"));
        return TBK_OK;
    }
    SpanRecorder* ev() { return &streams.used.back().ev; }  // of the handle staged last

    int upload(tbk_model* m) {
        TBK_HIP(hipMemcpyAsync(m->ws_mesh_k.ptr, h_k.data(), h_k.size() * sizeof(double), hipMemcpyHostToDevice, m->stream));
        return TBK_OK;
    }

    // The eigensystem, enqueued on the handle's stream (its device is current): with_u, tbk_eigh_device chunk by chunk (its own E, so
    // that E and U belong together), else the eigenvalue path alone.
    int fill(tbk_model* m, bool with_u) {
        const double* d_k = m->ws_mesh_k.as<double>();
        double *d_E = m->ws_mesh_e.as<double>(), *d_U = m->ws_mesh_u.as<double>();
        if (!with_u) return tbk_eigenval_device_hint(m, d_k, h_k.data(), nk, d_E);
        const size_t nn2 = (size_t)n_orb * n_orb * 2;
        const int64_t chunk = mesh_eigh_chunk(m, nk);
        for (int64_t c0 = 0; c0 < nk; c0 += chunk) {
            const int64_t nkc = std::min(chunk, nk - c0);
            TBK_CHECK(tbk_eigh_device(m, d_k + c0 * dim, nkc, 2, nullptr, d_E + (size_t)c0 * n_orb, d_U + (size_t)c0 * nn2));
        }
        return TBK_OK;
    }
};
