// tbk_dm.h -- what the calls that Fourier-transform matrices of a k mesh to lattice vectors share: tbk_dm.hip (the density matrix,
// real weights) and tbk_green.hip (the lattice Green's function, complex weights at a list of energies).  The mesh and the plan of
// one slab, the checks and the reduction of the lattice vectors, and the launchers of the three kernels both use: the phase table,
// the Fourier contraction and the sum of its k slices.  The kernels are in tbk_dm.hip (its head describes them and the table
// coordinates); the host drivers that launch them are tbk_lattice.hip's, and each family brings its own projector kernel, which
// writes the P operand of the contraction.
#pragma once

#include <vector>

#include "tbk_occ.h"

constexpr int DM_THREADS = 256;
constexpr size_t DM_PART_BUDGET = size_t(256) << 20;  // the partials of all slices together; fewer slices beyond it
constexpr size_t DM_TAB_BUDGET = size_t(256) << 20;   // the phase table of one chunk; a shorter chunk beyond it
constexpr int64_t DM_MAX_R = int64_t(65535) * 16;     // one grid row per 16 R-vectors

struct DmMesh {
    int dim;
    int n[3];       // (n[2] = 1 in two dimensions)
    int64_t nk;     // points of the whole mesh
    int64_t first;  // mesh index of the slab's first own point
};

struct DmPlan {
    DmMesh mesh;
    int n = 0;                       // orbitals
    int64_t n2 = 0, nct = 0;         // elements of one P (n^2; tbk_green.hip: of the energies of a tile), column tiles of 16 of them
    int64_t n_r = 0, nr_pad = 0;     // R-vectors, rounded up to the tile
    int64_t rows = 0;                // own mesh points of the slab
    int64_t slices = 1, kps = 4;     // k slices of the Fourier kernel, mesh points per slice (a multiple of 4)
    size_t part_bytes() const { return (size_t)slices * nr_pad * n2 * sizeof(double2); }
    size_t rho_bytes() const { return (size_t)n_r * n2 * sizeof(double2); }
    int64_t groups(int64_t chunk) const { return chunk / 4 + 2; }  // table groups of a chunk, at most
    size_t tab_bytes(int64_t chunk) const { return (size_t)nr_pad * groups(chunk) * 4 * 2 * sizeof(double); }
    size_t p_bytes(int64_t chunk) const { return (size_t)groups(chunk) * 4 * n2 * sizeof(double2); }
    // the same slab, slices and vectors with `elements` elements per table column
    DmPlan with_elements(int64_t elements) const {
        DmPlan L = *this;
        L.n2 = elements;
        L.nct = (elements + 15) / 16;
        return L;
    }
};

int dm_plan(int dim, const int32_t* mesh, int64_t nk_total, int64_t first_pt, int64_t rows, int n_orb, int64_t n_r, DmPlan* out);
// R[n_r][dim] reduced to [0, n_d) per axis
int dm_reduce_R(int dim, const int32_t* mesh, int64_t n_r, const int64_t* R, std::vector<int32_t>* out);
// a chunk no longer than the phase table's budget allows
int64_t dm_cap_chunk(const DmPlan& L, int64_t chunk);
int dm_check_R(int64_t n_r, const int64_t* R, const double* out, int n_orb);

// The slab's points [c0, c0 + nkc).  ev (may be NULL): the phase table is booked on stage 0, the contraction and the sum on stage 2.
// dm_launch_fourier: d_P is [table columns of the chunk][L.n2] complex, d_part [L.slices][L.nr_pad][L.n2] complex.
int dm_launch_phase(hipStream_t s, const DmPlan& L, SpanRecorder* ev, const int32_t* d_Rm, int64_t c0, int64_t nkc, double* d_tab);
int dm_launch_fourier(hipStream_t s, const DmPlan& L, SpanRecorder* ev, int64_t c0, int64_t nkc, const double* d_tab, const double2* d_P,
                      double2* d_part);
// the result of the slab in device memory: d_part itself with one slice, else the slices summed into d_rho
int dm_launch_reduce(hipStream_t s, const DmPlan& L, SpanRecorder* ev, const double2* d_part, double2* d_rho, const double2** result);
