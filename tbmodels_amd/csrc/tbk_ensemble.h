// tbk_ensemble.h -- what tbk_ensemble.hip (the transmission of an ensemble of devices) and tbk_channels.hip (its transmission
// eigenvalues) share on the host: the sizes of a call, the arguments of a launch, the rule that splits the samples into groups, and
// the two drivers -- the kernel alone on the caller's layers, and the whole call on one handle.  The drivers live in
// tbk_ensemble.hip and take the kernel as an EnsRoute, so that the chunks, the staging, the status words and the groups exist once.
#pragma once

#include "tbk_surface.h"

constexpr int64_t ENS_MAX_SAMPLES = 4096;  // samples per call (include/tbk.h); the status word gives the sample 12 bits

// The call's sizes, and the results of a chunk: T, iterations, the channels (tbk_channels.hip only: n doubles per sample), and behind
// them two status words -- the kernel's and the sweeps' of the library route in the first, the decimation of the library route
// (tbk_transmission's keys) in the second.
struct EnsShape {
    int n = 0, m_layers = 0;
    int64_t n_z = 0, n_s = 0;
    bool diag = false;
    bool channels = false;
    size_t device_bytes() const { return (size_t)n_s * m_layers * n * (diag ? sizeof(double) : (size_t)n * sizeof(double2)); }
    size_t t_bytes(int64_t nk) const { return surf_align256((size_t)nk * n_z * n_s * sizeof(double)); }
    size_t it_bytes(int64_t nk) const { return surf_align256((size_t)nk * n_z * sizeof(int32_t)); }
    size_t ch_bytes(int64_t nk) const { return channels ? surf_align256((size_t)nk * n_z * n_s * n * sizeof(double)) : 0; }
    size_t result_bytes(int64_t nk) const { return t_bytes(nk) + it_bytes(nk) + ch_bytes(nk); }
    static constexpr size_t flag_bytes = 2 * sizeof(unsigned long long);
    int64_t auto_chunk(int64_t nk) const {  // the chunk's results and its two layers inside the budget
        const size_t per_sample = sizeof(double) + (channels ? (size_t)n * sizeof(double) : 0);
        const size_t per_k = (size_t)n_z * ((size_t)n_s * per_sample + sizeof(int32_t)) + (size_t)2 * n * n * sizeof(double2);
        return std::max<int64_t>(1, std::min<int64_t>(nk, (int64_t)(SURF_CHUNK_BUDGET / per_k)));
    }
};

struct EnsLaunch {
    hipStream_t s;
    int n_cu;
    const double2 *d_H00, *d_H01;
    const void* d_V;
    const double2* d_z;
    int64_t nkc, sample_chunk;
    int max_it;
    unsigned long long key0;
    double* d_ws;
    int32_t* d_it;
    double* d_T;
    unsigned long long* d_flag;
    double* d_ch;  // [nkc][n_z][n_s][n] of a route with channels, else NULL
};

// A kernel of the family behind the drivers.  launch: the chunk's nkc points at every energy and sample on the own kernel.  The
// status word of the kernel is (key * radix + reason), key = (point index * 4096 + energy index) * 4096 + sample: radix 2 with the
// reasons 0 (a singular sweep) and 1 (the cap of the decimation), radix 4 with reason 2 (the cap of the channel iteration) besides.
struct EnsRoute {
    int (*launch)(const EnsShape&, const EnsLaunch&);
    unsigned radix;
    bool channels;  // the route writes channels; it takes N <= 64 only and has no library route
    int timed;      // the TimedFamily row of the whole call
    const char* family;
};

int tbk_ens_from_matrices(const EnsRoute& route, int device, int N, int64_t n_k, const double* H00, const double* H01, int M, int64_t n_s, const double* V,
                          const double* onsite, int64_t n_z, const double* z, int max_iterations, int64_t k_chunk, int64_t sample_chunk,
                          int32_t* iterations, double* T, double* channels);
int tbk_ens_slab(const EnsRoute& route, tbk_model* m, int64_t k_base, int axis, int layers, const double* k, int64_t nk, int M_device, int64_t n_s,
                 const double* V, const double* onsite, int64_t n_z, const double* z, int max_iterations, int32_t* iterations, double* T,
                 double* channels);

namespace {

// The groups: with sample_chunk = 0 the host takes G = min(n_s, ceil(R / (nkc n_z))) groups per (kp, z), R the workgroups resident at
// once (the CUs times the kernel's occupancy with its dynamic LDS; one per CU at NP = 64, as surf_grid assumes for the workspace
// slots), and ceil(n_s / G) samples per group: enough groups to fill the device and no more, because every group repeats the
// decimation.  The rule comes from the flop counts, not from a measurement.  spg: the samples of a group; no group
// is empty.
template <int NP>
int ens_sample_groups(const void* kernel, const EnsShape& sh, const EnsLaunch& a, int64_t& spg, int64_t& groups) {
    using Geo = SurfGeom<NP>;
    spg = std::min<int64_t>(a.sample_chunk, sh.n_s);
    if (a.sample_chunk == 0) {
        // R: the workgroups resident at once; G groups fill them and no more; the samples of a group
        int per_cu = 1;
        if (!Geo::GLOBAL) {
            TBK_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, Geo::THREADS, TransGeom<NP>::lds_bytes));
            per_cu = std::max(per_cu, 1);
        }
        const int64_t resident = (int64_t)std::max(a.n_cu, 1) * per_cu, kz = a.nkc * sh.n_z;
        const int64_t want = std::min<int64_t>(sh.n_s, (resident + kz - 1) / kz);
        spg = (sh.n_s + want - 1) / want;
    }
    groups = (sh.n_s + spg - 1) / spg;
    return TBK_OK;
}

}  // namespace
