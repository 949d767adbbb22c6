// tbk_tetra.h -- what the kernels that integrate over the simplices of a k mesh share: tbk_dos.hip (nos on an energy grid),
// tbk_pdos.hip (the projected one), tbk_fermi.hip (nos at probe energies) and tbk_occ.hip (the weight of every mesh point; tbk_occ.h
// carries its staged call on to tbk_dm.hip, the density matrix made from those weights).  Each
// of these is written ONCE here: the energy grid, the search on it and a workgroup's window; the fixed-point format of a
// contribution and the split of its 64-bit sums; the two sorts of a simplex's corners; the scaled gaps of a simplex with the
// number-of-states fraction n_T(E) and Bloechl's corner weights; the step from a work item to its cell's corner rows; and, on the
// host (tbk_dos.hip), the mesh and device checks, the geometry, the cut of the items into workgroups and the handles of a call on
// several devices with their slabs (the call itself, slab by slab: tbk_tetra_staged.h).  A kernel keeps what is its own: its loop
// over bins or probes, its loop over the simplices of a cell, its accumulators.
#pragma once

#include <algorithm>
#include <cmath>
#include <mutex>
#include <vector>

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

// A sum of fixed-point words, the high 44 and low 20 bits of every word apart: neither half overflows up to 2^20 words.
struct DosWords {
    unsigned long long hi = 0, lo = 0;
    __host__ __device__ __forceinline__ void add(unsigned long long word) {
        hi += word >> DOS_SPLIT_BITS;
        lo += word & ((1ull << DOS_SPLIT_BITS) - 1);
    }
    __device__ __forceinline__ double value() const {  // the sum / 2^40
        return (double)hi * (1.0 / (double)(1ull << (DOS_FRAC_BITS - DOS_SPLIT_BITS))) + (double)lo * (1.0 / (double)(1ull << DOS_FRAC_BITS));
    }
    // host: the sum as one integer, exactly; and an integer of words / 2^40 rounded to double once
    unsigned __int128 whole() const { return ((unsigned __int128)hi << DOS_SPLIT_BITS) + lo; }
    static double to_double(unsigned __int128 words) { return std::ldexp((double)words, -DOS_FRAC_BITS); }
};

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

// ---- the corners of a simplex in ascending order: NC = 4 (tetrahedron) or 3 (triangle) ------------------------------------------
__device__ __forceinline__ void tetra_sort2(double& a, double& b) {
    const double lo = fmin(a, b), hi = fmax(a, b);
    a = lo;
    b = hi;
}

// by value alone, for the kernels that need nothing but the sorted energies
template <int NC>
__device__ __forceinline__ void tetra_sort(double (&e)[NC]) {
    if constexpr (NC == 4) {
        tetra_sort2(e[0], e[1]);
        tetra_sort2(e[2], e[3]);
        tetra_sort2(e[0], e[2]);
        tetra_sort2(e[1], e[3]);
        tetra_sort2(e[1], e[2]);
    } else {
        tetra_sort2(e[0], e[1]);
        tetra_sort2(e[1], e[2]);
        tetra_sort2(e[0], e[1]);
    }
}

// Stable, for the kernels in which something belongs to a corner: adjacent exchanges on a strict comparison, so equal energies keep
// their order, and after every one the payload is told whether corners A and B = A + 1 changed places: payload.follow<A, B>(swapped)
template <int A, int B, int NC, class Payload>
__device__ __forceinline__ void tetra_exchange(double (&e)[NC], Payload& payload) {
    const bool sw = e[B] < e[A];
    const double lo = sw ? e[B] : e[A], hi = sw ? e[A] : e[B];
    e[A] = lo;
    e[B] = hi;
    payload.template follow<A, B>(sw);
}

template <int NC, class Payload>
__device__ __forceinline__ void tetra_stable_sort(double (&e)[NC], Payload& payload) {
    tetra_exchange<0, 1>(e, payload);
    tetra_exchange<1, 2>(e, payload);
    if constexpr (NC == 4) tetra_exchange<2, 3>(e, payload);
    tetra_exchange<0, 1>(e, payload);
    if constexpr (NC == 4) {
        tetra_exchange<1, 2>(e, payload);
        tetra_exchange<0, 1>(e, payload);
    }
}

// ---- the scaled gaps of one simplex ------------------------------------------------------------------------------------------------
// Built once per simplex from its SORTED corners: the corners times DOS_GAP_SCALE and the reciprocals of their differences, so that
// an evaluation costs multiplies and adds, no division.  Both members want e1 <= E < e_top: the ranges are half-open, the
// comparisons on the unscaled numbers select the branch, so a branch with a zero gap (reciprocal inf) is empty and never evaluated,
// and every ratio in [0, 1] is formed on its own.
template <int NC>
struct TetraGaps;

template <>
struct TetraGaps<4> {
    double e2, e3;
    double s1, s2, s3, s4;
    double r21, r31, r41, r32, r42, r43;
    __device__ __forceinline__ explicit TetraGaps(const double (&e)[4])
        : e2(e[1]),
          e3(e[2]),
          s1(e[0] * DOS_GAP_SCALE),
          s2(e[1] * DOS_GAP_SCALE),
          s3(e[2] * DOS_GAP_SCALE),
          s4(e[3] * DOS_GAP_SCALE),
          r21(1.0 / (s2 - s1)),
          r31(1.0 / (s3 - s1)),
          r41(1.0 / (s4 - s1)),
          r32(1.0 / (s3 - s2)),
          r42(1.0 / (s4 - s2)),
          r43(1.0 / (s4 - s3)) {}

    // n_T(E): the fraction of the tetrahedron below E
    __device__ __forceinline__ double fraction(double E) const {
        const double Es = E * DOS_GAP_SCALE;
        double n;
        if (E < e2) {
            const double x = Es - s1;
            n = (x * r21) * (x * r31) * (x * r41);
        } else if (E < e3) {
            const double x1 = Es - s1, x2 = Es - s2, y3 = s3 - Es, y4 = s4 - Es;
            const double q32 = x2 * r32;
            n = (x1 * r41) * (x1 * r31 + q32 * (y3 * r31)) + (x2 * r42) * q32 * (y4 * r41);
        } else {
            const double y = s4 - Es;
            n = 1.0 - (y * r41) * (y * r42) * (y * r43);
        }
        return n;
    }

    // Bloechl's weights of the four corners at E, in sorted order: they sum to n_T(E), a full corner is 1/4.
    // (Computed in four scalars and stored at the end, here and for the triangle: written into w[] inside the branches, the
    // merged values reach the caller's sum over the corners in another order, the compiler contracts another of its products into
    // an FMA, and pdos loses its bits in the last place.  tools/tetra_dump.py tells.)
    __device__ __forceinline__ void corner_weights(double E, double (&w)[4]) const {
        const double Es = E * DOS_GAP_SCALE;
        double w1, w2, w3, w4;
        if (E < e2) {
            const double x = Es - s1;
            const double q21 = x * r21, q31 = x * r31, q41 = x * r41;
            const double C = 0.25 * q21 * q31 * q41;
            w1 = C * (4.0 - (q21 + q31 + q41));
            w2 = C * q21;
            w3 = C * q31;
            w4 = C * q41;
        } else if (E < e3) {
            const double x1 = Es - s1, x2 = Es - s2, y3 = s3 - Es, y4 = s4 - Es;
            const double p31 = x1 * r31, p41 = x1 * r41, p32 = x2 * r32, p42 = x2 * r42;  // from below
            const double m31 = y3 * r31, m32 = y3 * r32, m41 = y4 * r41, m42 = y4 * r42;  // from above
            const double T = 0.25 * p41;
            const double C1 = T * p31;
            const double C2 = T * p32 * m31;
            const double C3 = 0.25 * p42 * p32 * m41;
            const double C12 = C1 + C2, C23 = C2 + C3, C123 = C12 + C3;
            w1 = C1 + C12 * m31 + C123 * m41;
            w2 = C123 + C23 * m32 + C3 * m42;
            w3 = C12 * p31 + C23 * p32;
            w4 = C123 * p41 + C3 * p42;
        } else {
            const double y = s4 - Es;
            const double q41 = y * r41, q42 = y * r42, q43 = y * r43;
            const double C = 0.25 * q41 * q42 * q43;
            w1 = 0.25 - C * q41;
            w2 = 0.25 - C * q42;
            w3 = 0.25 - C * q43;
            w4 = 0.25 - C * (4.0 - (q41 + q42 + q43));
        }
        w[0] = w1;
        w[1] = w2;
        w[2] = w3;
        w[3] = w4;
    }
};

template <>
struct TetraGaps<3> {
    double e2;
    double s1, s2, s3;
    double r21, r31, r32;
    __device__ __forceinline__ explicit TetraGaps(const double (&e)[3])
        : e2(e[1]),
          s1(e[0] * DOS_GAP_SCALE),
          s2(e[1] * DOS_GAP_SCALE),
          s3(e[2] * DOS_GAP_SCALE),
          r21(1.0 / (s2 - s1)),
          r31(1.0 / (s3 - s1)),
          r32(1.0 / (s3 - s2)) {}

    __device__ __forceinline__ double fraction(double E) const {
        const double Es = E * DOS_GAP_SCALE;
        double n;
        if (E < e2) {
            const double x = Es - s1;
            n = (x * r21) * (x * r31);
        } else {
            const double y = s3 - Es;
            n = 1.0 - (y * r31) * (y * r32);
        }
        return n;
    }

    // The weights of the three corners with a full corner worth 1 / FULL_DIV: 1/3 as they are, or 1 (every weight times three, so
    // that a full triangle is exact; the multiply by 1.0 folds away, and what is left is C = q21 * q31 and 1.0 - C * q31)
    template <int FULL_DIV = 3>
    __device__ __forceinline__ void corner_weights(double E, double (&w)[3]) const {
        const double full = 1.0 / FULL_DIV;
        const double Es = E * DOS_GAP_SCALE;
        double w1, w2, w3;
        if (E < e2) {
            const double x = Es - s1;
            const double q21 = x * r21, q31 = x * r31;
            const double C = full * q21 * q31;
            w1 = C * (3.0 - (q21 + q31));
            w2 = C * q21;
            w3 = C * q31;
        } else {
            const double y = s3 - Es;
            const double q31 = y * r31, q32 = y * r32;
            const double C = full * q31 * q32;
            w1 = full - C * q31;
            w2 = full - C * q32;
            w3 = full - C * (3.0 - (q31 + q32));
        }
        w[0] = w1;
        w[1] = w2;
        w[2] = w3;
    }
};

// ---- a work item: one (cell, band) pair, band fastest ------------------------------------------------------------------------------
struct TetraItem {
    int band;
    int i0, i1, i2;  // the cell (i0 < n0_cells)
    int j0, j1, j2;  // its neighbour along every axis, periodic over the planes held
};

__device__ __forceinline__ TetraItem tetra_item(const DosGeom& g, int64_t it) {
    TetraItem t;
    const int64_t cell64 = it / g.n_orb;
    t.band = (int)(it - cell64 * g.n_orb);
    int c = (int)cell64;  // NK < 2^31 (checked by the launcher)
    t.i2 = c % g.n2;
    c /= g.n2;
    t.i1 = c % g.n1;
    t.i0 = c / g.n1;
    t.j0 = t.i0 + 1 == g.n0_planes ? 0 : t.i0 + 1;
    t.j1 = t.i1 + 1 == g.n1 ? 0 : t.i1 + 1;
    t.j2 = t.i2 + 1 == g.n2 ? 0 : t.i2 + 1;
    return t;
}

// the row of mesh point (a0, a1, a2) in E (and W)
__device__ __forceinline__ int64_t tetra_row(const DosGeom& g, int a0, int a1, int a2) { return ((int64_t)a0 * g.n1 + a1) * g.n2 + a2; }

// ---- host (tbk_dos.hip) ------------------------------------------------------------------------------------------------------------
inline size_t dos_align256(size_t x) { return (x + 255) / 256 * 256; }

// the text of dos, pdos and the Fermi level for a wrong dim
inline constexpr const char* DOS_MESH = "the density of states needs a 2- or 3-dimensional mesh";
// dim in {2, 3} (`what`: the caller's text for a wrong one), mesh not NULL, every entry >= 1, *nk_total = points of the mesh < 2^31
int tetra_check_mesh(int dim, const int32_t* mesh, const char* what, int64_t* nk_total);
// ... and the grid checks every density-of-states entry point shares
int tbk_dos_check(int dim, const int32_t* mesh, double e_step, int64_t n_e, const void* nos_out, int64_t* nk_total);
// a visible device of that index, made current
int tetra_check_device(int device);
// cells0 cells along axis 0 out of planes0 planes held in E (planes0 == cells0: the axis wraps onto itself); items_per_wg is left 0
DosGeom tetra_geom(int dim, const int32_t* mesh, int64_t cells0, int64_t planes0, int n_orb);
// Workgroups of `threads` threads: enough to give every thread an item, no more than cap, never more than DOS_MAX_ITEMS items each
// nor more than 2^DOS_SPLIT_BITS workgroups (`what`: the caller's text for a mesh that needs more)
int tetra_partition(int64_t items, int threads, int64_t cap, const char* what, int64_t* items_per_wg, int* n_wg);
// the k list of `planes` planes of axis 0 from plane p_lo on (periodic), in mesh order: k_d = i_d / n_d
int tbk_dos_mesh_klist(int dim, const int32_t* mesh, int64_t p_lo, int64_t planes, std::vector<double>* h_k);
// The eigenvalues of those planes on a staged handle, enqueued on its stream: the k list goes through ws_k, the eigenvalues stay in
// ws_out (the eigenvalue path with the host list as the fold hint: dense models fold, CSR models take their own path).  below: the
// periodic neighbour plane p_lo - 1 too, from a second call, in front of the others in h_k, ws_k and ws_out.  The caller has made
// the handle's device current and reserved its family's workspaces (the eigenvalue call chooses its chunk from what is left), keeps
// h_k until it has called tbk_eigenval_check, and calls that: callers with several handles enqueue all of them first.
int tbk_mesh_eigenvalues(tbk_model* m, const int32_t* mesh, int64_t p_lo, int64_t planes, bool below, std::vector<double>* h_k);

// n0 rows (planes of axis 0, or k-points) on n handles: handle i takes the ceil(n0 / n) from lo(i) on, the last handles possibly none
struct TetraSlabs {
    int64_t n0, per;
    TetraSlabs(int64_t n0_, int n) : n0(n0_), per((n0_ + n - 1) / n) {}
    int64_t lo(int i) const { return std::min<int64_t>(n0, (int64_t)i * per); }
    int64_t count(int i) const { return std::min<int64_t>(n0, lo(i) + per) - lo(i); }
    int busy() const { return (int)((n0 + per - 1) / std::max<int64_t>(per, 1)); }  // handles whose slab is not empty
};

// The handles of one mesh call on staged models.  open() checks them (none, NULL, of different models, k.p, one twice) and the mesh,
// and takes every handle's lock, in address order, until the object goes.
struct TetraHandles {
    std::vector<std::unique_lock<std::recursive_mutex>> locks;
    int dim = 0, n_orb = 0;
    int64_t nk_total = 0, plane_pts = 0;
    TetraSlabs cut{0, 1};  // of axis 0 among the handles
    int open(tbk_model* const* handles, int n_handles, const int32_t* mesh, const char* what);
};
