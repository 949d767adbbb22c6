// tbk_tetra_staged.h -- the scaffold of a tetrahedron call on staged handles: the handles checked and locked, axis 0 of
// the mesh cut into slabs, per busy handle the family's reservations and the eigenvalues of its slab's planes with their periodic
// neighbour plane(s), every handle checked.  tbk_dos.hip, tbk_pdos.hip, tbk_fermi.hip and tbk_occ.h (weights, occupations, and through
// them tbk_dm.hip and tbk_chi.hip) each add their launches and their sum over the slabs; the wait on every exit and the booking of the
// kernel times are MeshStreams' (tbk_resident.h).  Beside it the one step the entry points on the caller's arrays share.
#pragma once

#include <vector>

#include "tbk_resident.h"

// One handle's slab of the mesh: the cells of `p_count` planes of axis 0 from p_lo on.  Its eigenvalues hold one periodic neighbour
// plane more behind the own ones (the last cells' corners) and, for a family that asks for it, one in front (the first points'
// simplices) -- unless the slab is the whole axis, which wraps onto itself.
struct TetraSlab {
    tbk_model* m = nullptr;
    int64_t p_lo = 0, p_count = 0;
    int64_t planes = 0;           // of axis 0 in d_E
    int off0 = 0;                 // the first own plane among them
    int64_t head = 0;             // the mesh points in front of the own ones in d_E and in the handle's k list: off0 planes
    const double* d_E = nullptr;  // [planes * plane_pts][n_orb], in the handle's ws_out
    std::vector<double> h_k;      // the k list of those planes, the source of an enqueued copy
    SpanRecorder* ev = nullptr;   // the handle's recorder in TetraStaged::streams

    void cut(int64_t n0, int64_t lo, int64_t count, bool below, int64_t plane_pts) {
        const bool whole = count == n0;
        p_lo = lo;
        p_count = count;
        off0 = below && !whole ? 1 : 0;
        planes = (whole ? n0 : count + 1) + off0;
        head = off0 * plane_pts;
    }
    int64_t upper_planes() const { return planes - off0; }  // the own planes and the neighbour behind them
    const double* own_E(int n_orb) const { return d_E + (size_t)head * n_orb; }
};

// Handle i takes slab i of TetraHandles::cut; handles whose slab is empty are skipped.  The calling thread holds every handle's lock
// for the whole call and drives all of them.  `streams` waits when it goes, so a host buffer that an enqueued copy reads or writes is
// a member in front of it (the slabs' h_k) or lives in an object declared IN FRONT of the staged one -- never in a member of a
// derived type, which goes before the wait (OccStaged: a base in front of this one).  DESIGN 13.6 lists every family's.
struct TetraStaged : TetraHandles {
    std::vector<TetraSlab> slabs;
    MeshStreams streams;  // (behind the slabs: it waits before their host buffers go)

    // reserve(slab, index): the family's plan and reservations on the handle, whose device is current -- in front of the eigenvalues,
    // which size their chunk from what is free then.  below: the neighbour plane in front too.  own_fill (make_slab): reserve enqueues
    // the slab's eigenvalues itself (pdos: E and U of one eigenvector call belong together), d_E is for it to set.
    template <class Reserve>
    int make(tbk_model* const* handles, int n_handles, const int32_t* mesh, const char* what, bool below, Reserve&& reserve) {
        TBK_CHECK(open(handles, n_handles, mesh, what));
        slabs.resize((size_t)cut.busy());
        for (int i = 0; i < cut.busy(); ++i) TBK_CHECK(enqueue(i, handles[i], mesh, cut.lo(i), cut.count(i), below, reserve, false));
        return streams.check();
    }

    // The slab [lo, lo + count) alone, on one handle: for the two calls whose _multi form runs one host thread per handle, each with a
    // staged object of its own (dos, pdos: DESIGN 13.6 has the measurement that kept the threads)
    template <class Reserve>
    int make_slab(tbk_model* m, const int32_t* mesh, const char* what, int64_t lo, int64_t count, Reserve&& reserve, bool own_fill) {
        TBK_CHECK(open(&m, 1, mesh, what));
        slabs.resize(1);
        TBK_CHECK(enqueue(0, m, mesh, lo, count, false, reserve, own_fill));
        return streams.check();
    }

private:
    template <class Reserve>
    int enqueue(int i, tbk_model* m, const int32_t* mesh, int64_t lo, int64_t count, bool below, Reserve&& reserve, bool own_fill) {
        TetraSlab& s = slabs[(size_t)i];
        s.m = m;
        TBK_CHECK(streams.add(m));
        s.ev = &streams.used.back().ev;
        s.cut(mesh[0], lo, count, below, plane_pts);
        TBK_CHECK(reserve(s, (size_t)i));
        if (own_fill) return TBK_OK;
        TBK_CHECK(tbk_mesh_eigenvalues(m, mesh, s.p_lo, s.upper_planes(), s.off0 != 0, &s.h_k));
        s.d_E = m->ws_out.as<double>();
        return TBK_OK;
    }
};

// The slabs' shares of a result of n doubles (dos, pdos): the host buffer the handles' copies go to -- the caller declares it in front of
// its TetraStaged -- and their sum in handle order
inline int tetra_shares(std::vector<double>* share, size_t doubles) {
    try {
        share->assign(doubles, 0.0);
    } catch (...) {
        tbk_set_error("cannot allocate the per-handle results");
        return TBK_ERR_MEMORY;
    }
    return TBK_OK;
}
inline void tetra_add_shares(const std::vector<double>& share, size_t slabs, size_t n, double* out) {
    for (size_t j = 0; j < n; ++j) {
        double sum = share[j];
        for (size_t i = 1; i < slabs; ++i) sum += share[i * n + j];
        out[j] = sum;
    }
}

// ---- tbk_fermi.hip on a slab ---------------------------------------------------------------------------------------------------------
constexpr int FERMI_PROBES = 16;  // probe energies per launch

struct FermiLaunch {
    DosGeom g;
    int n_wg = 0, edge_wg = 0;
    int64_t rows = 0;  // mesh rows of this slab's own cells (without the periodic neighbour plane)
    size_t off_count = 0, off_sums = 0, off_pmin = 0, off_pmax = 0, off_emin = 0, off_emax = 0, ws_bytes = 0;
};

// The Fermi state of one slab: where its eigenvalues and its workspace are, and the host side of the copies a pass enqueues.  A
// call keeps these in a vector declared IN FRONT of its TetraStaged, whose streams wait before the vector goes.
struct FermiSlab {
    int device = 0, dim = 0;
    hipStream_t stream = nullptr;
    FermiLaunch L;
    const double* d_E = nullptr;  // the slab's own planes first, the neighbour plane behind them
    char* d_ws = nullptr;
    SpanRecorder* ev = nullptr;  // NULL: not timed (the caller's eigenvalues; a search on behalf of another family)
    unsigned long long h_sums[FERMI_PROBES * 3];
    std::vector<double> h_edges;  // emin, emax [2][n_orb]
};

// The Fermi search (mode 1, value = n_electrons: mu, lower, upper, N(mu) of tbk_fermi) or N at one energy (mode 0, value = the energy:
// mu = lower = upper = value) on the eigenvalues a staged call keeps: the slabs as they are, `state` the caller's vector in front of
// `staged`.  The probe rows go through every handle's ws_dos; the kernels are not booked.  tbk_occupations, the density matrix and
// the susceptibilities find their mu here.
int tbk_fermi_resident(TetraStaged& staged, std::vector<FermiSlab>& state, const int32_t* mesh, int mode, double value, double* out4);
int tbk_fermi_check_electrons(double n_electrons, int n_orb);

// E[nk][n_orb] of the caller on the device that tetra_check_device has just made current
struct TetraOwnedE {
    DevBuf buf;
    size_t bytes = 0;
    int upload(const double* E, int64_t nk, int n_orb) {
        bytes = (size_t)nk * (size_t)n_orb * sizeof(double);
        TBK_CHECK(buf.reserve(bytes));
        TBK_HIP(hipMemcpy(buf.ptr, E, bytes, hipMemcpyHostToDevice));
        return TBK_OK;
    }
    const double* d() const { return buf.as<double>(); }
};
