// tbk_dos_common.h -- what the density-of-states kernels (tbk_dos.hip) and the projected ones (tbk_pdos.hip) share: the energy
// grid, the search on it, the window of a workgroup and the fixed-point format of a contribution.  One definition, so both
// kernels select the same bins and the same branch at every grid point.
#pragma once

#include "tbk_internal.h"

// Fixed point: a contribution in [0, 1] is stored as round(x * 2^40), i.e. with an error of at most 2^-41 each.
constexpr int DOS_FRAC_BITS = 40;
// the reduction over workgroups splits every 64-bit bin into its high 44 and low 20 bits and sums each in 64 bits: exact up to
// 2^20 workgroups (the launchers never take more than that)
constexpr int DOS_SPLIT_BITS = 20;
constexpr int64_t DOS_MAX_ITEMS = int64_t(1) << 20;  // (cell, band) pairs per workgroup
constexpr int64_t DOS_MAX_NE = int64_t(1) << 20;     // documented limit of the energy grid (tbk.h)

struct DosGeom {
    int n0_cells;   // cells along axis 0 this launch covers
    int n0_planes;  // planes of axis 0 in E: n0_cells + 1 for a slab (its periodic neighbour plane is the last), n0_cells for a whole mesh
    int n1, n2;     // the other axes (n2 = 1 in two dimensions)
    int n_orb;
    int64_t items;         // n0_cells * n1 * n2 * n_orb
    int64_t items_per_wg;  // contiguous items per workgroup, <= DOS_MAX_ITEMS
};

struct DosWindow {
    double e_min, e_step, inv_step;
    int n_e;
    int tile_lo, tile_n;  // this workgroup's bins
};

__device__ __forceinline__ double dos_grid(double e_min, double e_step, int j) {
    // two roundings, never an FMA: the same number as NumPy's e_min + j * e_step
    return __dadd_rn(e_min, __dmul_rn((double)j, e_step));
}

// first j in [0, n_e] with E_j >= e (n_e: none).  The multiply gives a guess, the comparisons decide.  NaN -> 0, no iteration.
__device__ __forceinline__ int dos_first_at_or_above(double e, double e_min, double e_step, double inv_step, int n_e) {
    double t = ceil((e - e_min) * inv_step);
    t = fmin(fmax(t, 0.0), (double)n_e);
    int j = (int)t;
    while (j > 0 && dos_grid(e_min, e_step, j - 1) >= e) --j;
    while (j < n_e && dos_grid(e_min, e_step, j) < e) ++j;
    return j;
}

// x in [0, 1] (clamped; NaN -> 0) as fixed point
__device__ __forceinline__ unsigned long long dos_fixed(double x) {
    x = fmin(fmax(x, 0.0), 1.0);
    return (unsigned long long)__double2ll_rn(x * (double)(1ull << DOS_FRAC_BITS));
}

// Branch arithmetic.  Every branch of the tetrahedron formulas is a polynomial in ratios x / gap in [0, 1], x a
// distance of E from a corner and gap the corner difference that contains it, and the kernels form every ratio on its own as
// x * (1 / gap): a product of three small distances can then not underflow to 0 against a product of reciprocals that overflowed.
// What is left is a gap whose own reciprocal overflows -- below about 2^-1024, deep in the subnormal range, which starts under
// 2^-1022 -- where x = 0 would give 0 * inf; so
// the corner energies and E are multiplied by DOS_GAP_SCALE first.  That is exact (a power of two), the ratios do not change, and
// the smallest positive gap, 2^-1074, becomes 2^-1020 with a finite reciprocal.  Only the reciprocal of a ZERO gap is inf, and a
// branch that is selected has none (the comparisons are made on the unscaled numbers).  Energies above 2^969 would overflow
// (include/tbk.h states the limit).
constexpr double DOS_GAP_SCALE = 0x1p54;

inline size_t dos_align256(size_t x) { return (x + 255) / 256 * 256; }

// tbk_dos.hip: the checks every density-of-states entry point shares (*nk_total = points of the whole mesh), and the k list of
// `planes` planes of axis 0 from plane p_lo on (periodic), in mesh order: k_d = i_d / n_d
int tbk_dos_check(int dim, const int32_t* mesh, double e_step, int64_t n_e, const void* nos_out, int64_t* nk_total);
int tbk_dos_mesh_klist(int dim, const int32_t* mesh, int64_t p_lo, int64_t planes, std::vector<double>* h_k);
