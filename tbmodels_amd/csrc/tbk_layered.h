// tbk_layered.h -- the host side of the calls on the stacked-layer geometry: the surface Green's function, the
// transmission, the device Green's function and the bond currents, the transmission of an ensemble and its eigenvalues.  Two drivers
// in tbk_layered.hip serve all of them -- the kernel alone on the caller's layers, and the whole call on one handle -- with the
// chunks, the staging, the status words and the timer stages; a family describes itself to them as a LayeredFamily.  The host
// helpers of the geometry and surface_layers_kernel live beside the drivers, once.
#pragma once

#include "tbk_surface.h"

// One chunk as a family's kernel sees it.
struct LayeredChunk {
    hipStream_t s;                 // the handle's stream; NULL on the caller's layers
    int n_cu;
    rocblas_handle blas;           // the library route's (the handle's, or the call's own)
    const double2 *d_H00, *d_H01;  // [nkc][N][N]; d_H01 NULL: no hopping between the layers
    const void* d_V;               // the staged potential, NULL where the family has none
    const double2* d_z;
    char* d_ws;                    // workspace_bytes of the route
    char* d_extra;                 // extra_bytes
    int64_t nkc, k0;               // the chunk's points; the index of its first in the caller's list: key0 = k0 * SURF_MAX_Z
    int max_it;
    char* d_res;                   // result_bytes(nkc) and, behind them, the status words
};

// a chunk's results to the host: enqueued on the handle's stream, or synchronous
struct LayeredCopy {
    hipStream_t s;
    bool async;
    hipError_t operator()(void* dst, const void* src, size_t bytes) const {
        return async ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s) : hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
    }
};

// What a family supplies.  The texts and sizes are set by its constructor; check() learns the rows N of a principal layer, fills the
// family's shape and sets h_V and v_bytes, so every other member is asked after it.
struct LayeredFamily {
    const char* family = nullptr;  // in the reservations' messages: "the transmission of an ensemble"
    const char* needs = nullptr;   // in "... needs hopping / a tight-binding model": "the transmission"
    TimedFamily timed = TIMED_SURFACE;
    int min_layers = 1;                                  // 0: a call without hopping between the layers is served (H01 NULL)
    int rows_clamp = 1 << 20;                            // surf_check_energies sees min(N, rows_clamp): below it the family's own bound speaks
    int64_t max_points = int64_t(1) << 40;               // n_k and nk stay below it, so that the keys fit the status word ...
    bool base_counts = false;                            // ... and k_base + nk does, with k_base >= 0
    const char *bad_n_k = "n_k < 1", *bad_nk = "nk < 0";
    int n_words = 1;                                     // status words behind a chunk's results
    const void* h_V = nullptr;                           // the potential staged once per call: host pointer, bytes, the reservation's text
    size_t v_bytes = 0;
    const char* v_what = "the device potential";
    const char* extra_what = nullptr;

    virtual int check(int N) = 0;                         // the family's checks behind the energies' (and H01's), in its order
    virtual int check_options() const { return TBK_OK; }  // ... and of the options only *_from_matrices takes
    virtual size_t result_bytes(int64_t nk) const = 0;
    virtual int64_t auto_chunk(int64_t nk) const = 0;
    virtual bool library(int eigensolver) const = 0;
    virtual size_t workspace_bytes(bool library, int64_t chunk, int n_cu) const = 0;
    virtual size_t extra_bytes(int64_t /*chunk*/, int /*n_cu*/) const { return 0; }  // a second buffer per launch (ws_mesh_u)
    virtual int run_chunk(bool library, const LayeredChunk& c) const = 0;
    virtual int copy_out(const LayeredCopy& copy, const char* d_res, int64_t nkc, int64_t c0) const = 0;
    virtual unsigned long long chunk_word(const unsigned long long* words) const { return words[0]; }  // a chunk's words as one
    virtual int status_error(unsigned long long word, const double* z, int max_iterations) const = 0;
    virtual ~LayeredFamily() = default;
};

// The family's kernel alone on principal layers the caller brings (the tbk_*_from_matrices entry points): the null stream,
// synchronous copies, TBK_EIG_AUTO decides the route and the call owns the library's handle.
int layered_from_matrices(LayeredFamily& fam, int device, int N, int64_t n_k, const double* H00, const double* H01, int64_t n_z, const double* z,
                          int max_iterations, int64_t k_chunk);

// The whole call on one handle for the k-points [k_base, k_base + nk) of a longer list (the slabs of the *_multi calls): the messages
// name k_base + the point's index.
int layered_slab(LayeredFamily& fam, tbk_model* m, int64_t k_base, int axis, int layers, const double* k, int64_t nk, int64_t n_z, const double* z,
                 int max_iterations);

// what every call checks of its sizes, energies and cap
int surf_check_energies(int N, int64_t n_z, const double* z, int max_iterations);
// what the calls with a device check of it; M N^2 complex numbers are staged once per call
int trans_check_device(int N, int M, const double* V, const int32_t* iterations, const double* T);
// the status word as an error: the first (point, energy) of the call that failed
int surf_status_error(unsigned long long word, const double* z, int max_iterations, const char* what = "z - e of the decimation");
