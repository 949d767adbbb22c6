// tbk_lattice.h -- the host side of the calls that Fourier-sum a matrix P(k) of a uniform k mesh into lattice vectors R (DESIGN.md
// 20.8): the density matrix rho(R) (tbk_dm.hip), the lattice Green's function G(R, z) and the dressed one (tbk_green.hip).  Two
// drivers in tbk_lattice.hip serve all of them -- on the caller's arrays, and one slab on one staged handle -- with the plan, the
// reservations, the chunks, the tiles of energies and the timer stages.  A family describes itself to them as a LatticeFamily and
// brings the step that fills P; the kernels the drivers launch themselves are tbk_dm.h's.
#pragma once

#include "tbk_dm.h"

constexpr int GREEN_ZT = 4;                         // energies per tile, at most: green_project_kernel keeps their accumulators in registers
constexpr int64_t GREEN_MAX_Z = 4096;               // energies per call (include/tbk.h)
constexpr size_t GREEN_P_BUDGET = size_t(1) << 30;  // the P of one chunk and one tile
constexpr unsigned long long GREEN_NO_FLAG = ~0ull;

// One slab: the density matrix's plan for n^2 elements (its slices are those of every family, whatever the energies), the k chunk,
// the energy tile and the tiles of the call.  The density matrix is the case of one energy in one tile whose result is the sum of
// the slices itself (gather false).
struct GreenPlan {
    DmPlan D;
    int64_t n_z = 1, zt = 1, tiles = 1, chunk = 1;
    int bt = 4;          // the projector template
    bool gather = true;  // the tiles' sums are put side by side into G [n_r][n_z][n^2]
    int64_t tile_count(int64_t t) const { return std::min(zt, n_z - t * zt); }
    DmPlan tile_plan(int64_t t) const { return D.with_elements(tile_count(t) * D.n2); }
    size_t part_stride() const { return D.with_elements(zt * D.n2).part_bytes(); }  // between the partials of two tiles
    size_t part_bytes() const { return (size_t)tiles * part_stride(); }
    size_t p_bytes() const { return D.with_elements(zt * D.n2).p_bytes(chunk); }
    size_t g_bytes() const { return (size_t)D.n_r * n_z * D.n2 * sizeof(double2); }
    size_t sum_bytes() const { return D.slices > 1 ? D.with_elements(zt * D.n2).rho_bytes() : 0; }  // the sum of one tile's slices
    size_t sum_offset() const { return gather ? dos_align256(g_bytes()) : 0; }                     // ... behind G, where there is one
    size_t result_bytes() const { return sum_offset() + sum_bytes(); }
    size_t in_bytes(bool needs_h) const { return ((size_t)chunk * D.n2 * 2 + (needs_h ? 0 : (size_t)chunk * D.n)) * sizeof(double); }
};

// k_chunk > 0: the caller's chunk, and the tile is what keeps its P inside the budget; 0: the tile is z_tile (0: GREEN_ZT) and the
// chunk min(auto_chunk, what the budget allows that tile).  The tile does not depend on auto_chunk.
GreenPlan green_plan(const DmPlan& D, int64_t n_z, int64_t z_tile, int64_t k_chunk, int64_t auto_chunk);

// One chunk as the step that fills P sees it: the slab's points [c0, c0 + nkc), table column j is chunk point j - pad.
struct LatticeChunk {
    hipStream_t s;  // the handle's stream; NULL on the caller's arrays
    const GreenPlan& G;
    int64_t c0, nkc, pad, ng;      // ng groups of four table columns; (ng, 1) or (4 ng, blocks of 64 x 64) workgroups project them
    double* d_in;                  // [G.chunk][n][n] complex: U, with the eigenvalues [G.chunk][n] behind it, or the full H(k)
    const double2 *d_z, *d_sigma;  // the call's energies [n_z] and self-energy [n_z][n][n], where the family has them
    unsigned long long* d_flag;    // the status word
    rocblas_handle blas;           // the library route's (the handle's, or the call's own); NULL: the own kernels
    char* d_work;                  // work_bytes of the route
    double2* d_P;                  // [table columns][energy in tile][n][n]
    double* d_E() const { return d_in + (size_t)G.chunk * G.D.n2 * 2; }
    dim3 project_grid() const { return G.bt == 1 ? dim3((unsigned)ng, 1) : dim3((unsigned)(ng * 4), (unsigned)(((G.D.n + 63) / 64) * ((G.D.n + 63) / 64))); }
};

// What a family supplies; its entry points set the call's arguments (dim and mesh: the drivers do).
struct LatticeFamily {
    TimedFamily timed;
    int dim = 0;
    const int32_t* mesh = nullptr;
    // in the message of a reservation that does not fit: the family ("the Green's function") and what the buffer keeps; NULL: the plain message
    const char *family = nullptr, *part_what = nullptr, *result_what = nullptr, *const_what = nullptr, *in_what = nullptr, *p_what = nullptr,
               *work_what = nullptr;
    bool needs_h = false;                           // a chunk's P is made from the full H(k) of chunk_h, not from the eigensystem of tbk_eigh_device
    bool has_status = false;                        // a status word comes down with the result and goes through status_error
    int64_t n_z;                                    // the call's energies ...
    const double *z, *sigma;                        // ... staged behind the lattice vectors: z, then the self-energy (NULL: none)

    LatticeFamily(TimedFamily timed_, int64_t n_z_ = 1, const double* z_ = nullptr, const double* sigma_ = nullptr)
        : timed(timed_), n_z(n_z_), z(z_), sigma(sigma_) {}
    virtual GreenPlan plan(const DmPlan& D, int64_t z_tile, int64_t k_chunk, int64_t auto_chunk) const { return green_plan(D, n_z, z_tile, k_chunk, auto_chunk); }
    virtual int share(int zt, bool library) const = 0;  // buffers of the chunk's size beside its eigenvectors (mesh_eigh_chunk)
    virtual bool library(int /*n_orb*/, int /*eigensolver*/) const { return false; }
    virtual size_t work_bytes(const GreenPlan& /*G*/) const { return 0; }  // of the library route
    virtual int fill_p(const LatticeChunk& c, int64_t tile) const = 0;     // P of one tile of energies: stage 1 of the timer
    virtual int status_error(unsigned long long /*word*/) const { return TBK_OK; }
    virtual ~LatticeFamily() = default;
};

// What one call on staged handles keeps on the host: the buffers that enqueued copies read and write -- the reduced lattice vectors,
// the slabs' k lists, the results of the slabs behind the first, the status words.  A MeshStreams waits for its handles when it goes,
// so this object is declared IN FRONT of it (or of the OccStaged that holds it): what is declared behind is destroyed before the wait.
struct LatticeCall {
    int64_t n_r = 0;
    double* out = nullptr;
    size_t out_doubles = 0;
    std::vector<int32_t> h_Rm;
    std::vector<std::vector<double>> h_k, partial;
    std::vector<unsigned long long> words;
    int open(LatticeFamily& fam, const TetraHandles& th, const int32_t* mesh, int64_t n_r_, const int64_t* R, double* out_, size_t slabs);
};

// The family's call on arrays the caller brings, behind the entry point's checks (the device's last): the null stream, synchronous
// copies, the call's own buffers; TBK_EIG_AUTO decides the route and the call owns the library's handle.  A chunk uploads its rows
// of E [nk][n] (NULL: none) and of mat, U or H [nk][n][n] complex.
int lattice_from_arrays(LatticeFamily& fam, int dim, const int32_t* mesh, int64_t nk, int n_orb, const double* E, const double* mat, int64_t k_chunk,
                        int64_t z_tile, int64_t n_r, const int64_t* R, double* out);

// Slab `slab` of the call on handle m (its device current, ev its recorder): nk mesh points from mesh index first_pt on, d_k their k
// list on the device.  Everything from the plan to the enqueued download into call.out (slab 0) or call.partial[slab].
int lattice_slab(LatticeFamily& fam, const TetraHandles& th, LatticeCall& call, size_t slab, tbk_model* m, SpanRecorder* ev, const double* d_k,
                 int64_t nk, int64_t first_pt);

// The end of a call on handles: synchronises every handle (the eigenvector flags are reported as by tbk_eigh) and books the kernel
// times; then the status words, the smallest first; then the slabs' results summed in handle order.
int lattice_finish(const LatticeFamily& fam, LatticeCall& call, MeshStreams& streams);
