// tbk_occ.h -- what the calls that integrate with the point weights w[k][b] of a mesh share: tbk_occ.hip (weights, occupations) and
// tbk_dm.hip (the real-space density matrix).  The plan of one slab, the launchers of tbk_occ.hip's kernels, and the staged call:
// TetraStaged (tbk_tetra_staged.h: the handles with their slabs and the slabs' eigenvalues), then mu and the weights.  The kernels
// are in tbk_occ.hip; the check of every handle, the finish and the wait on every exit are MeshStreams' (tbk_resident.h).
#pragma once

#include <algorithm>
#include <vector>

#include "tbk_tetra_staged.h"

struct OccGeom {
    int n0_own;     // planes of axis 0 this launch writes weights for
    int n0_planes;  // planes of axis 0 in E
    int off0;       // the first own plane in E: 0 for a whole mesh, 1 for a slab with its two neighbour planes
    int n1, n2;     // the other axes (n2 = 1 in two dimensions)
    int n_orb;
    int64_t items;  // n0_own * n1 * n2 * n_orb
};

// ---- host: one slab of the mesh on one device ----------------------------------------------------------------------------------
struct OccPlan {
    OccGeom g;
    int dim = 0;
    int64_t rows = 0;      // own mesh points
    int64_t n_blocks = 0;  // of the band sums
    int64_t kpw = 1, n_wg = 1;
    int w_grid = 1;
    // the workspace: part_f, part_eb [n_blocks][n]; buf [n_wg][n]; then what goes to the host in one copy: f high / low [2][n],
    // q high / low [2][n] (u64), eb [n] (double)
    size_t off_part_eb = 0, off_buf = 0, off_host = 0, host_bytes = 0, ws_bytes = 0;
};

// cells0 own planes along axis 0 out of planes0 planes in E, the first own one at off0
int occ_plan(int dim, const int32_t* mesh, int64_t cells0, int64_t planes0, int off0, int n_orb, OccPlan* out);
int occ_launch_weights(hipStream_t s, const OccPlan& L, const double* d_E, double mu, double nk_total, double* d_w);
// d_E_own: the rows of E of the own mesh points
int occ_launch_band(hipStream_t s, const OccPlan& L, const double* d_w, const double* d_E_own, double nk_total, char* ws);
int occ_clear_buf(hipStream_t s, const OccPlan& L, char* ws);
// the own points [c0, c0 + nkc) of the slab: d_U their eigenvectors, d_w the slab's weights
int occ_launch_contract(hipStream_t s, const OccPlan& L, const double* d_U, const double* d_w, int64_t c0, int64_t nkc, double nk_total, char* ws);
int occ_launch_reduce(hipStream_t s, const OccPlan& L, char* ws);

inline constexpr const char* OCC_MESH ="the tetrahedron weights need a 2- or 3-dimensional mesh";

// ---- the mesh on staged handles ------------------------------------------------------------------------------------------------
// what a slab keeps beside TetraSlab.  The stages of its recorder: 0 the weights kernel, 1 the band sums, 2 the contraction + its
// reduction (tbk_dm.hip: its own three)
struct OccSlab {
    OccPlan L;
    std::vector<double> host;  // the off_host block
};

// the host side of what the call enqueues: a base in front of TetraStaged, so that it goes after the streams have waited
struct OccHost {
    std::vector<OccSlab> occ;      // beside TetraStaged::slabs
    std::vector<FermiSlab> fermi;  // find_mu's passes
};

// Handle i takes the slab of tbk_dos_multi.  Its eigenvalues: the planes [p_lo, p_lo + p_count] come from ONE call of the
// eigenvalue path on the k list tbk_fermi_multi gives it (the same call, so the same bits: mu is tbk_fermi's), the neighbour plane
// p_lo - 1 from a second call, in front of them in ws_out.  A handle that holds the whole axis needs neither neighbour.
struct OccStaged : OccHost, TetraStaged {
    // the handles and the mesh, checked and locked; then the eigenvalues of every slab, checked
    int make(tbk_model* const* handles, int n_handles, const int32_t* mesh) {
        return TetraStaged::make(handles, n_handles, mesh, OCC_MESH, true, [&](TetraSlab& s, size_t i) -> int {
            occ.resize(i + 1);  // (nothing is enqueued into these before the eigenvalues are checked)
            OccPlan& L = occ[i].L;
            TBK_CHECK(occ_plan(dim, mesh, s.p_count, s.planes, s.off0, n_orb, &L));
            TBK_CHECK(s.m->ws_occ_w.reserve((size_t)L.rows * n_orb * sizeof(double)));
            return s.m->ws_occ.reserve(L.ws_bytes);
        });
    }

    // mode 1: the Fermi search of tbk_fermi on the resident eigenvalues; mode 0: N(value) from the probe kernel
    int find_mu(const int32_t* mesh, int mode, double value, double* mu_out) { return tbk_fermi_resident(*this, fermi, mesh, mode, value, mu_out); }

    // timed: the kernel is booked on stage 0 of the slab's recorder (not for a caller whose stages are others)
    int weights(double mu, double* w_out, bool timed = true) {
        for (size_t i = 0; i < slabs.size(); ++i) {
            TetraSlab& s = slabs[i];
            const OccPlan& L = occ[i].L;
            TBK_HIP(hipSetDevice(s.m->device));
            if (timed) s.ev->start(0);
            TBK_CHECK(occ_launch_weights(s.m->stream, L, s.d_E, mu, (double)nk_total, s.m->ws_occ_w.as<double>()));
            if (timed) s.ev->stop();
            if (w_out)
                TBK_HIP(hipMemcpyAsync(w_out + (size_t)s.p_lo * plane_pts * n_orb, s.m->ws_occ_w.ptr, (size_t)L.rows * n_orb * sizeof(double),
                                       hipMemcpyDeviceToHost, s.m->stream));
        }
        return TBK_OK;
    }

    // f, eb and q of every slab (the weights are in ws_occ_w), left in occ[i].host
    int sums() {
        for (size_t i = 0; i < slabs.size(); ++i) {
            TetraSlab& s = slabs[i];
            const OccPlan& L = occ[i].L;
            tbk_model* m = s.m;
            TBK_HIP(hipSetDevice(m->device));
            char* ws = m->ws_occ.as<char>();
            const double* d_w = m->ws_occ_w.as<double>();
            s.ev->start(1);
            TBK_CHECK(occ_launch_band(m->stream, L, d_w, s.own_E(n_orb), (double)nk_total, ws));
            s.ev->stop();
            TBK_CHECK(occ_clear_buf(m->stream, L, ws));
            // the chunk's eigenvalues (not used: the weights come from the eigenvalue path) go behind its eigenvectors
            const int64_t nk = L.rows;
            const int64_t chunk = mesh_eigh_chunk(m, nk);
            const size_t u_doubles = (size_t)chunk * n_orb * n_orb * 2;
            TBK_CHECK(m->ws_pdos_u.reserve((u_doubles + (size_t)chunk * n_orb) * sizeof(double)));
            double* d_U = m->ws_pdos_u.as<double>();
            const double* d_k_own = m->ws_k.as<double>() + (size_t)s.head * dim;
            for (int64_t c0 = 0; c0 < nk; c0 += chunk) {
                const int64_t nkc = std::min(chunk, nk - c0);
                TBK_CHECK(tbk_eigh_device(m, d_k_own + c0 * dim, nkc, 2, nullptr, d_U + u_doubles, d_U));
                s.ev->start(2);
                TBK_CHECK(occ_launch_contract(m->stream, L, d_U, d_w, c0, nkc, (double)nk_total, ws));
                s.ev->stop();
            }
            s.ev->start(2);
            TBK_CHECK(occ_launch_reduce(m->stream, L, ws));
            s.ev->stop();
            try {
                occ[i].host.resize(5 * (size_t)n_orb);
            } catch (...) {
                tbk_set_error("cannot allocate the per-handle results");
                return TBK_ERR_MEMORY;
            }
            TBK_HIP(hipMemcpyAsync(occ[i].host.data(), ws + L.off_host, L.host_bytes, hipMemcpyDeviceToHost, m->stream));
        }
        return TBK_OK;
    }

    // synchronises every handle (the eigenvector flags are reported as by tbk_eigh) and books the kernel times
    int finish(TimedFamily family = TIMED_OCC) { return streams.finish(family); }
};
