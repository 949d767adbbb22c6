// tbk_ensemble.h -- what tbk_ensemble.hip (the transmission of an ensemble of devices) and tbk_channels.hip (its transmission
// eigenvalues) share on the host: the sizes of a call, the arguments of a launch, the rule that splits the samples into groups, and
// EnsFamily, which describes either kernel to the drivers of tbk_layered.h (its members live in tbk_ensemble.hip).
#pragma once

#include "tbk_layered.h"

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
    size_t t_bytes(int64_t nk) const { return dos_align256((size_t)nk * n_z * n_s * sizeof(double)); }
    size_t it_bytes(int64_t nk) const { return dos_align256((size_t)nk * n_z * sizeof(int32_t)); }
    size_t ch_bytes(int64_t nk) const { return channels ? dos_align256((size_t)nk * n_z * n_s * n * sizeof(double)) : 0; }
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

// A kernel of the family.  launch: the chunk's nkc points at every energy and sample on the own kernel.  The status word of the
// kernel is (key * radix + reason), key = (point index * 4096 + energy index) * 4096 + sample: radix 2 with the reasons 0 (a singular
// sweep) and 1 (the cap of the decimation), radix 4 with reason 2 (the cap of the channel iteration) besides.
struct EnsRoute {
    int (*launch)(const EnsShape&, const EnsLaunch&);
    unsigned radix;
    bool channels;  // the route writes channels; it takes N <= 64 only and has no library route
    TimedFamily timed;
    const char* family;
};

// The ensemble's calls as a LayeredFamily: the samples staged once per call in either form, two status words per chunk (EnsShape).
// sample_chunk: the option of *_from_matrices, 0 on a handle.
struct EnsFamily : LayeredFamily {
    const EnsRoute& route;
    EnsShape sh;
    const double *V, *onsite;
    int64_t sample_chunk;
    int32_t* iterations;
    double *T, *channels;
    EnsFamily(const EnsRoute& route, int M, int64_t n_s, const double* V, const double* onsite, int64_t n_z, int64_t sample_chunk, int32_t* iterations,
              double* T, double* channels);
    int check(int N) override;
    int check_options() const override;
    size_t result_bytes(int64_t nk) const override { return sh.result_bytes(nk); }
    int64_t auto_chunk(int64_t nk) const override { return sh.auto_chunk(nk); }
    bool library(int eigensolver) const override { return !route.channels && surf_takes_library(sh.n, eigensolver); }
    size_t workspace_bytes(bool library, int64_t chunk, int n_cu) const override;
    int run_chunk(bool library, const LayeredChunk& c) const override;
    int copy_out(const LayeredCopy& copy, const char* d_res, int64_t nkc, int64_t c0) const override;
    unsigned long long chunk_word(const unsigned long long* words) const override;
    int status_error(unsigned long long word, const double* z, int max_iterations) const override;
};

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
