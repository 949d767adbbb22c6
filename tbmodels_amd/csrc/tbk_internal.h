// tbk_internal.h -- shared declarations of libtbk.so (not part of the C ABI; see include/tbk.h).
#pragma once

#include <hip/hip_runtime.h>
#include <rocblas/rocblas.h>

#include <atomic>
#include <cstdlib>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "tbk.h"

// ------------------------------------------------------------------------------------------------
// Tile geometry of the dense H(k) kernel (tbk_hk_dense.hip).  The staging code pads to these.
// ------------------------------------------------------------------------------------------------
constexpr int TBK_BM = 128;      // k-points per workgroup tile
constexpr int TBK_BNP = 64;      // packed (i <= j) matrix elements per workgroup tile (x2 real columns)
constexpr int TBK_BK = 16;       // depth of one LDS stage in real K rows (= 8 lattice vectors)
constexpr int TBK_CT = 16;       // packed elements per MFMA column tile
constexpr int TBK_MAX_DIM = 8;   // lattice dimension limit of the phase kernel

// Packed slots of the dense operand (d_colmap): (i << 16) | j for the element H[i][j], i <= j, one real column per plane
// (Re, Im); -1 for padding.  Tight-binding models put TWO diagonal elements in one slot, (i << 16) | TBK_SLOT_PAIR | j:
// plane 0 is Re H[i][i], plane 1 Re H[j][j] (their Im parts are 0 by construction and not contracted), so N orbitals
// take N (N - 1) / 2 + ceil(N / 2) = ceil(N^2 / 2) slots instead of N (N + 1) / 2.  j < 32768: bit 15 is free.
constexpr int32_t TBK_SLOT_PAIR = 0x8000;

// ------------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------------
void tbk_set_error(const char* fmt, ...);

#define TBK_HIP(expr)                                                                             \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            tbk_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__,        \
                          __LINE__);                                                              \
            return (e_ == hipErrorOutOfMemory) ? TBK_ERR_MEMORY : TBK_ERR_DEVICE;                 \
        }                                                                                         \
    } while (0)

#define TBK_ROCBLAS(expr)                                                                         \
    do {                                                                                          \
        rocblas_status s_ = (expr);                                                               \
        if (s_ != rocblas_status_success) {                                                       \
            tbk_set_error("%s failed: rocblas_status %d (%s:%d)", #expr, (int)s_, __FILE__,       \
                          __LINE__);                                                              \
            return (s_ == rocblas_status_memory_error) ? TBK_ERR_MEMORY : TBK_ERR_DEVICE;         \
        }                                                                                         \
    } while (0)

#define TBK_CHECK(expr)                                                                           \
    do {                                                                                          \
        int r_ = (expr);                                                                          \
        if (r_ != TBK_OK) return r_;                                                              \
    } while (0)

#define TBK_LOCK(m) std::lock_guard<std::recursive_mutex> tbk_lock_((m)->mu)

#define TBK_ARG(cond, msg)                                                                        \
    do {                                                                                          \
        if (!(cond)) {                                                                            \
            tbk_set_error("invalid argument: %s", msg);                                           \
            return TBK_ERR_ARGUMENT;                                                              \
        }                                                                                         \
    } while (0)

// ------------------------------------------------------------------------------------------------
// Environment switches.  The library reads only the switches a test uses as an independent cross-check of the product path
// (TBK_BAND, TBK_BAND_SPLIT, TBK_BAND_XL, TBK_BAND_XL_FROM, TBK_CHASE_WINDOW, TBK_REG128, TBK_REG128_NW2,
// TBK_GATHER_BLOCK_ROWS -- the table in DESIGN.md section 6).  The seven eigensolver switches are read once per process by
// tbk_eig_env (tbk_eig_plan.hip) and consulted by tbk_eig_plan alone; TBK_GATHER_BLOCK_ROWS is read in tbk_comm.hip.  Variants
// that were built, measured and dropped are not in the sources; their measurements are in DESIGN_LOG.md and their code in the
// git history.
// ------------------------------------------------------------------------------------------------
struct tbk_eig_env_t {  // TBK_BAND, _BAND_SPLIT, _BAND_XL, _CHASE_WINDOW, _REG128, _REG128_NW2 (0: off), TBK_BAND_XL_FROM=n
    bool band = true, band_split = true, band_xl = true, chase_window = true, reg128 = true, reg128_nw2 = true;
    int band_xl_from = 1024;
};
const tbk_eig_env_t& tbk_eig_env();

// ------------------------------------------------------------------------------------------------
// dynamic LDS above the 64 KiB default: hipFuncSetAttribute acts on the CURRENT device's copy of the
// kernel, so it is raised once per (kernel instantiation, device) -- `done` is that instantiation's flag row.
// ------------------------------------------------------------------------------------------------
constexpr int TBK_MAX_DEVICES = 64;

// (the flags are atomics: two handles on one device -- Model.devices = [0, 0] -- launch from two host threads)
using tbk_flag_row = std::atomic<bool>[TBK_MAX_DEVICES];
inline hipError_t tbk_raise_lds_limit(const void* kernel, int bytes, tbk_flag_row& done) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev >= 0 && dev < TBK_MAX_DEVICES && done[dev].load(std::memory_order_acquire)) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess && dev >= 0 && dev < TBK_MAX_DEVICES) done[dev].store(true, std::memory_order_release);
    return e;
}

// ------------------------------------------------------------------------------------------------
// Owners of GPU resources.  Move-only; each converts to its raw handle or pointer, so launches, copies and
// hipStreamWaitEvent / hipEventRecord take them as they take the raw ones.  put(): the address a create call fills (what
// the owner held before is let go first).  Members are destroyed with the struct that holds them: nothing else frees.
// ------------------------------------------------------------------------------------------------
template <class H, auto Destroy>
struct Owned {
    H h = nullptr;
    Owned() = default;
    Owned(Owned&& o) noexcept : h(o.h) { o.h = nullptr; }
    Owned& operator=(Owned&& o) noexcept {
        if (this != &o) {
            reset();
            h = o.h;
            o.h = nullptr;
        }
        return *this;
    }
    Owned(const Owned&) = delete;
    Owned& operator=(const Owned&) = delete;
    ~Owned() { reset(); }
    void reset() {
        if (h) (void)Destroy(h);
        h = nullptr;
    }
    H* put() {
        reset();
        return &h;
    }
    operator H() const { return h; }
};
template <class T>
using DevPtr = Owned<T*, hipFree>;  // device memory of hipMalloc
using PinnedPtr = Owned<void*, hipHostFree>;
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using Event = Owned<hipEvent_t, hipEventDestroy>;

// a grow-only device buffer
struct DevBuf {
    DevPtr<void> ptr;
    size_t bytes = 0;
    int reserve(size_t want);  // keeps contents only if no reallocation happens
    template <class T>
    T* as() const {
        return static_cast<T*>(ptr.h);
    }
};
static_assert(!std::is_copy_constructible<DevBuf>::value && !std::is_copy_assignable<DevBuf>::value,
              "a DevBuf owns its memory: it moves, it is never copied");

// ------------------------------------------------------------------------------------------------
// HIP-event timing.  One span: the kernels between a start and a stop event on one stream, booked on `stage`.
// ------------------------------------------------------------------------------------------------
struct EventSpan {
    Event start, stop;
    int stage = 0;
};

// The spans of one call on one stream.  start / stop do nothing when timing is off; collect, after the stream has been
// synchronised, adds every span to ms[stage] and drops the spans.  An event that cannot be created or read switches the
// recorder off for good (`on` tells): the call goes on untimed and what it had recorded is not added.
struct SpanRecorder {
    hipStream_t stream = nullptr;
    bool on = false;
    std::vector<EventSpan> spans;
    SpanRecorder() = default;
    SpanRecorder(bool timing, hipStream_t s) : stream(s), on(timing) {}
    void start(int stage = 0);
    void stop();
    void collect(double* ms);
};

// The sums the mesh calls book their kernel times on, one row per family (tbk_dos_timing, tbk_pdos_timing, tbk_fermi_timing,
// tbk_occ_timing, tbk_dm_timing, tbk_chi_timing, tbk_berry_timing, tbk_green_timing, tbk_green_dressed_timing, tbk_surface_timing, tbk_transmission_timing, tbk_device_green_timing, tbk_device_current_timing, tbk_transmission_ensemble_timing, tbk_transmission_channels_timing, tbk_optics_timing, tbk_tdf_timing: what each counts differs and is
// listed in DESIGN.md section 10)
enum TimedFamily { TIMED_DOS, TIMED_PDOS, TIMED_FERMI, TIMED_OCC, TIMED_DM, TIMED_CHI, TIMED_BERRY, TIMED_GREEN, TIMED_DYSON, TIMED_SURFACE, TIMED_TRANSMISSION, TIMED_DEVICE_GREEN, TIMED_DEVICE_CURRENT, TIMED_TRANSMISSION_ENSEMBLE, TIMED_TRANSMISSION_CHANNELS, TIMED_OPTICS, TIMED_TDF, TIMED_COUNT };
struct TimedSums {
    double ms[3] = {0.0, 0.0, 0.0};  // per stage of the family (dos and fermi have one, occ, dm, chi, berry, green, the dressed green, surface, transmission, the device green, the device current, the ensemble, the channels, the optical conductivity and the transport distribution three)
    int64_t calls = 0;
    int64_t passes = 0;  // fermi: the passes of its searches
};

// ------------------------------------------------------------------------------------------------
// The right-hand side of one H(k) contraction: a lattice and the operand rows staged for it.  The staged operand of a
// model (tbk_staged_operand, below) or a folded one (tbk_fold_plan_t::operand); tbk_hk_plan stores the one its chunk takes.
// ------------------------------------------------------------------------------------------------
struct tbk_operand_t {
    int dim = 0;
    int64_t n_r = 0, n_r_pad = 0, k2 = 0;
    const int32_t* d_R = nullptr;   // [n_r_pad][dim], NULL for k.p
    const double* d_B = nullptr;    // Bt[k2][ncol_pad / 16][2][16]
};

// ------------------------------------------------------------------------------------------------
// folding along one k component (tbk_fold.hip)
// ------------------------------------------------------------------------------------------------
struct tbk_fold_plan_t {
    bool built = false;
    int dim = 0;                 // dimension of the lattice this plan folds (the folded one has dim - 1)
    int64_t n_r = 0;             // its lattice vectors
    int64_t n_rho = 0, n_rho_pad = 0, k2 = 0;  // folded lattice vectors; K rows of the folded operand
    int64_t row_len = 0;         // doubles per operand row: ncol_pad * 2
    int capacity = 0;            // folded operands that fit d_B2
    std::vector<int32_t> h_R2;   // host copy of the folded lattice [n_rho][dim - 1] (second-level plans are built on it)
    DevPtr<int32_t> d_R2;        // [n_rho_pad][dim - 1]
    DevPtr<int64_t> d_lptr;      // [n_rho_pad + 1] lists of contributing lattice vectors
    DevPtr<int32_t> d_lrec;      // r | (negated ? 1 << 31 : 0)
    DevPtr<int32_t> d_rcomp;     // [n_r] the folded component of every lattice vector
    DevPtr<double> d_B2;         // [capacity][k2][row_len] folded operands
    DevPtr<double> d_table;      // [n_r][slots][2] (cos, sin) of the shared-component phases
    int64_t table_entries = 0;   // its capacity in (r, slot) pairs
    std::unique_ptr<tbk_fold_plan_t[]> sub;  // [dim - 1] second-level plans (mesh lines inside a mesh plane), built on demand
    double* slot(int s) const { return d_B2 + (size_t)s * k2 * row_len; }
    // the folded model whose operand rows are in slot s
    tbk_operand_t operand(int s) const { return {dim - 1, n_rho, n_rho_pad, k2, d_R2, slot(s)}; }
};

// ------------------------------------------------------------------------------------------------
// staged model
// ------------------------------------------------------------------------------------------------
struct tbk_model {
    // One host thread at a time per handle: the entry points share workspaces, the fold cache and the stage timers
    // (ctypes drops the GIL for the duration of a call).  Recursive: the host-buffer calls go through the device ones.
    std::recursive_mutex mu;
    int device = 0;
    int n_cu = 256;  // compute units of the device (workgroup slots per round = 2 * n_cu for the H(k) kernel)
    // dim, n_r, n_r_pad, k2, d_R, d_B are the staged operand: written by creation and staging (tbk_api.hip create_common,
    // tbk_stage.hip), read-only from then on
    int dim = 0;
    int n_orb = 0;
    int64_t n_r = 0;
    bool sparse = false;
    bool kdotp = false;  // K rows are k.p monomials (one per Taylor coefficient) instead of phases

    // --- common staging ---
    int64_t n_r_pad = 0;   // n_r rounded up so that 2 * n_r_pad is a multiple of TBK_BK
    int64_t k2 = 0;        // real K rows of the contraction: 2 * n_r_pad (cos, sin per lattice vector)
    int ncol = 0;          // packed slots: ceil(n_orb^2 / 2) for dense tight-binding models (diagonal pairs),
                           // n_orb (n_orb + 1) / 2 upper-triangle elements for CSR and k.p models
    int ncol_pad = 0;      // rounded up to TBK_BNP
    DevPtr<int32_t> d_R;       // [n_r_pad][dim] lattice vectors (padding rows are zero)
    DevPtr<int32_t> d_colmap;  // [ncol_pad]  (i << 16) | j, (i << 16) | TBK_SLOT_PAIR | j, or -1 for padding
    DevPtr<int32_t> d_powers;  // k.p only: [n_r][dim] monomial exponents

    // --- dense: symmetrised hop planes, tile-interleaved  Bt[K2][ncol_pad / 16][2][16] ---
    DevPtr<double> d_B;
    // --- dense, n_r_pad >= TBK_STRASSEN_MIN_NR: the seven right operands of one Strassen level, Bs[7][K2 / 2][ncol_pad / 2 / 16][2][16]
    // (tbk_stage.hip), built from the staged d_B and valid for that operand alone (a folded one has none)
    DevPtr<double> d_Bs;
    // --- the 49 right operands of two Strassen levels, Bs2[49][K2 / 4][ncol_pad / 4 / 16][2][16]: the table applied to each block
    // of d_Bs (valid while d_Bs is).  Built by the first call whose chunks take two levels (tbk_stage_strassen2); bs2_skipped:
    // they did not fit a quarter of the free memory then, and the model stays on one level
    DevPtr<double> d_Bs2;
    bool bs2_skipped = false;

    // --- sparse: per packed element, the list of lattice vectors that touch it ---
    int64_t nnz_rec = 0;
    DevPtr<int64_t> d_cptr;   // [ncol + 1]
    DevPtr<int32_t> d_rec_r;  // [nnz_rec]  (kind << 28) | r   kind: 0 direct, 1 transposed, 2 diagonal
    DevPtr<double> d_rec_v;   // [nnz_rec][2]
    // the same records in the order the LDS kernel walks them: per 64 packed elements ("wave round") a number of steps,
    // every step one record (or none) per lane, arranged so that the 16 lanes the LDS serves together read 16 different
    // 16-byte slots of its 256-byte row (tbk_hk_csr.hip: tbk_csr_schedule)
    int sched_kt = 0;             // k-points per phase tile the schedule was built for (0: no schedule)
    int64_t sched_steps = 0;
    DevPtr<int64_t> d_sptr;    // [ceil(ncol / 64) + 1] first step of every wave round
    DevPtr<int32_t> d_srec_r;  // [sched_steps][64]  (sign code << 30) | byte offset of the phase row, 0x80000000: no record
    DevPtr<double> d_srec_v;   // [sched_steps][64][2]

    int64_t staged_bytes = 0;

    // --- folding (k lists with long runs of one shared component) ---
    std::vector<int32_t> h_R;  // host copy of the lattice vectors [n_r][dim]
    tbk_fold_plan_t fold[TBK_MAX_DIM];
    bool fold_enabled = true;
    bool strassen = true;  // TBK_OPT_STRASSEN
    int strassen_levels = 2;  // TBK_OPT_STRASSEN_LEVELS
    bool strassen_combine_split = true;  // TBK_OPT_STRASSEN_COMBINE
    int64_t counters[TBK_CNT_COUNT] = {0, 0, 0, 0, 0, 0, 0};  // tbk_model_counter

    // --- options ---
    int eigensolver = TBK_EIG_AUTO;
    int64_t k_chunk = 0;
    bool timing = false;

    // --- runtime ---
    // (members are destroyed last to first: the streams are declared in front of everything that is used on them, and the
    // rocBLAS handle, behind them, goes before the stream it was set to; tbk_model_destroy synchronises the streams first)
    Stream stream;      // phase rows, H(k), rocSOLVER, collectives
    Stream stream_eig;  // wave eigensolver: reduction to tridiagonal form
    Stream stream_ql;   // wave eigensolver: tridiagonal QL (latency-bound, overlaps the rest)
    Stream stream_xl[3];  // band_xl_* above 1024 orbitals: the other groups of a batch (tbk_eig_band.hip)
    Event ev_xl[4];     // fork, and one join per extra group
    Event ev_hk[2];     // H[buf] written
    Event ev_tri[2];    // H[buf] consumed, (d, e)[buf] written
    Event ev_out[2];    // tbk_hamilton: chunk in ws_out / ws_out2 computed
    Event ev_ql[2];     // (d, e)[buf] consumed, eigenvalues written
    Event ev_s2[2];     // two-pass Strassen combine (launch_strassen2): the first product launch done, the first pass done
    Event ev_sync;      // host waits on the main stream go through this event (tbk_api.hip)
    Owned<rocblas_handle, rocblas_destroy_handle> blas;
    DevBuf ws_phase;  // [K2][nk_pad] cos/sin rows
    DevBuf ws_H;      // [chunk][n_orb][n_orb] complex
    DevBuf ws_H2;     // second H buffer: folded H(k) of a chunk is built beside the previous chunk's reduction
    DevBuf ws_E;      // rocSOLVER: [chunk][n_orb] off-diagonal scratch; wave solver: (d, e) of buffer 0
    DevBuf ws_E2;     // wave solver: (d, e) of buffer 1
    DevBuf ws_info;   // [chunk] int
    DevBuf ws_k;      // host-entry staging of k / pos / E
    DevBuf ws_pos;
    DevBuf ws_orb;    // convention 1: orbital phase table of the current chunk
    DevBuf ws_out;
    DevBuf ws_out2;  // second device buffer of the chunked H(k) download (tbk_hamilton)
    DevBuf ws_flag;   // int[2]: {non-convergence count, non-finite count}
    // small host-buffer calls (one k-point per call is what Z2Pack-style callers do): k, the result and the flags cross
    // PCIe through this PINNED buffer -- asynchronous DMA copies enqueued back to back and ONE synchronisation, where
    // three copies from / to pageable memory each cost a host-side staging round trip (~20 us apiece)
    PinnedPtr h_stage;
    size_t h_stage_bytes = 0;
    DevBuf ws_part;   // split-K partial tiles of the dense H(k) kernel (small k batches)
    DevBuf ws_c11;    // two-pass Strassen combine: the four partial C11 quarters between its passes, [4][Mq][ncol_pad / 4] (re, im)
    DevBuf ws_kfold;  // k-points of a folded run without the folded component
    DevBuf ws_kline;  // one mesh line without both folded components (second-level fold)
    DevBuf ws_band;   // two-stage reduction: pending [V | W] panel of every matrix of a chunk
    DevBuf ws_bandmat[2];  // ... and the band matrices between its stages (one per chunk in flight)
    // one-k host calls (tbk_one_k_t): the convention-1 positions stay on the device between calls (uploaded again when their bytes change)
    std::vector<double> pos_cache;  // host copy of what ws_posraw holds
    DevBuf ws_posraw;
    DevBuf ws_xl;     // the launch chain of band_xl_*: the second matrix buffer (the sweep of a panel reads one, writes the other)
    // The tetrahedron calls on staged handles (TetraStaged, tbk_tetra_staged.h): a slab's k list goes through ws_k and its eigenvalues
    // stay in ws_out, for every family
    DevBuf ws_dos;    // tbk_dos / tbk_pdos: the workgroups' fixed-point bins [n_wg][NE], the combined bins and nos (tbk_dos.hip, tbk_pdos.hip);
                      // tbk_fermi and every search for mu (tbk_fermi_resident: occupations, density matrix, susceptibilities): its rows and partials
    DevBuf ws_pdos_u;    // the eigenvectors of one k chunk [chunk][n_orb][n_orb] complex: tbk_pdos; tbk_occupations, with the chunk's
                         // eigenvalues behind them (the R-space calls of tbk_lattice.hip: below)
    DevBuf ws_pdos_w;    // tbk_pdos: the weights of the whole slab W[NK][G][n_orb]
    DevBuf ws_pdos_grp;  // ... the groups: offsets [G + 1] and, 256-byte aligned behind them, the orbital list
    DevBuf ws_occ_w;     // the point weights of the slab's own mesh points w[rows][n_orb] (tbk_occ.hip): tbk_tetra_weights, tbk_occupations,
                         // tbk_density_matrix
    DevBuf ws_occ;       // tbk_occupations: the block partials of the band sums, the workgroups' rows of the contraction and the combined words
    // The calls that Fourier-sum a matrix of the mesh into lattice vectors (lattice_slab, tbk_lattice.hip): tbk_density_matrix,
    // tbk_green_function, tbk_green_dressed.  The chunk's eigenvectors, with their eigenvalues behind them, or its full H(k) go
    // through ws_pdos_u, the Green's functions' k list through ws_mesh_k, the dressed one's library batch, pivots and status
    // through ws_mesh_work.
    DevBuf ws_dm_r;      // the lattice vectors reduced modulo the mesh, int32 [n_r][dim]; 256-byte aligned behind them the energies [n_z]
                         // and the self-energy [n_z][n_orb][n_orb], both complex
    DevBuf ws_dm_tab;    // the phase table of one k chunk, [R tiles][groups of 4 k][cos | sin][64]
    DevBuf ws_dm_p;      // P of one k chunk and one tile of energies, [table columns][energy in tile][n_orb][n_orb] complex
    DevBuf ws_dm_part;   // per tile the k slices' partial sums [slices][n_r padded to 16][energy in tile][n_orb][n_orb] complex, across the chunks
    DevBuf ws_dm_rho;    // rho: their sum [n_r][n_orb][n_orb] complex (more than one slice); G [n_r][n_z][n_orb][n_orb], behind it one tile's sum
                         // The layered calls (layered_slab, tbk_layered.hip) use the same buffers: ws_mesh_k the k list with its
                         // samples along the stacking axis, ws_dm_r energies and twiddles, ws_pdos_u H(k) of one chunk, ws_dm_p its
                         // principal layers, ws_dm_rho its results and status words, ws_mesh_work the workgroups' slots or the library
                         // route's batch; with a device, ws_mesh_io its potential V (tbk_transmission_ensemble,
                         // tbk_transmission_channels: the devices of all samples, in either form); tbk_device_green and
                         // tbk_device_current: ws_mesh_u the workgroups' stacks
    DevBuf ws_green_flag;  // tbk_green_dressed: one 64-bit status word, all ones or the smallest (mesh index * 4096 + energy index) that was singular
    // The calls on the resident eigensystem of a whole mesh (tbk_resident.h; the susceptibilities of tbk_chi.hip, tbk_berry_flux of
    // tbk_berry.hip): k, E and U are ResidentMesh's, the other two each family lays out for itself
    DevBuf ws_mesh_k;     // the k list of the whole mesh [NK][dim]
    DevBuf ws_mesh_e;     // the eigenvalues of the whole mesh [NK][n_orb]; chi: behind them the Fermi tables f, 1 - f [2][NK][n_orb]
    DevBuf ws_mesh_u;     // the eigenvectors of the whole mesh [NK][n_orb][n_orb] complex (chi: with matrix elements; berry: always)
    DevBuf ws_mesh_io;    // the call's arguments and results on this handle.  chi: the results of its vectors (double [n_q], complex
                          // [n_q][n_w] or [n_q][m][m]) and the frequencies [n_w], 256-byte aligned behind them the phases D [n_q][n_orb]
                          // complex (convention 1), the reduced q int32 [n_q][3], the orbital selection int32 [2][m].  berry: the links
                          // L [sets][dim][k share] complex, their words (u64) and |L|, each 256-byte aligned, then the phases D [dim][n_orb]
    DevBuf ws_mesh_work;  // the call's partials or workspace.  chi: the partial sums of one batch of vectors, [batch][NK][blocks],
                          // complex [batch][w_pass][NK][blocks] or [batch][slices][mp][mp].  berry: (handle 0) the plaquette kernel's
                          // outputs and, with several handles, the words and |L| of the whole mesh; behind them the library path's batch
    std::vector<EventSpan> events;  // StageTimer's spans, read by tbk_get_timing (no synchronisation on the pipeline's path)
    double t_ms[TBK_T_COUNT] = {0, 0, 0, 0};
    int64_t t_n[TBK_T_COUNT] = {0, 0, 0, 0};
    TimedSums timed[TIMED_COUNT];
};

// the operand the model was staged with
inline tbk_operand_t tbk_staged_operand(const tbk_model* m) { return {m->dim, m->n_r, m->n_r_pad, m->k2, m->d_R, m->d_B}; }

struct tbk_kdotp {
    tbk_model* core = nullptr;  // the dense pipeline with monomial rows in place of phase rows
};

// what a tbk_*_timing getter does behind its argument checks: the family's row (its first `stages` times; passes may be NULL),
// read and, if asked, reset under the handle's lock
int tbk_timed_read(tbk_model* m, TimedFamily family, int stages, double* ms, int64_t* calls, int64_t* passes, int reset);

// tbk_surface.hip: tbk_surface_green on one handle for the k-points [k_base, k_base + nk) of a longer list (the slabs of
// tbk_surface_green_multi): the messages name k_base + the point's index
int tbk_surface_green_slab(tbk_model* m, int64_t k_base, int axis, int layers, const double* k, int64_t nk, int64_t n_z, const double* z,
                           int max_iterations, int spectral, int32_t* iterations, double* bottom, double* top, double* bulk);

// ... and tbk_transmission in the same way (the slabs of tbk_transmission_multi)
int tbk_transmission_slab(tbk_model* m, int64_t k_base, int axis, int layers, const double* k, int64_t nk, int M, const double* V, int64_t n_z,
                          const double* z, int max_iterations, int32_t* iterations, double* T, double* G);

// tbk_ensemble.hip: tbk_transmission_ensemble in the same way (the slabs of tbk_transmission_ensemble_multi)
int tbk_transmission_ensemble_slab(tbk_model* m, int64_t k_base, int axis, int layers, const double* k, int64_t nk, int M, int64_t n_s, const double* V,
                                   const double* onsite, int64_t n_z, const double* z, int max_iterations, int32_t* iterations, double* T);

// tbk_channels.hip: tbk_transmission_channels in the same way (the slabs of tbk_transmission_channels_multi)
int tbk_transmission_channels_slab(tbk_model* m, int64_t k_base, int axis, int layers, const double* k, int64_t nk, int M, int64_t n_s, const double* V,
                                   const double* onsite, int64_t n_z, const double* z, int max_iterations, int32_t* iterations, double* T,
                                   double* channels);

// tbk_surface.hip: the library route of the ensemble for tbk_ensemble.hip -- the bytes of its workspace d_ws, and one chunk of nkc
// points on it.  Exactly one of d_V ([n_s][m_layers][n][n] complex) and d_onsite ([n_s][m_layers][n]) is not NULL; d_T: [nkc][n_z][n_s];
// d_flag: two words, the sweeps' (keys with the sample) and the decimation's (the keys of tbk_transmission)
size_t tbk_trans_ens_lib_bytes(int n);
int tbk_trans_ens_lib_chunk(hipStream_t s, rocblas_handle blas, char* d_ws, int n, int m_layers, int64_t n_s, const double2* d_H00, const double2* d_H01,
                            const double2* d_V, const double* d_onsite, const double2* d_z, int64_t n_z, int64_t nkc, int max_it, int64_t k0, int32_t* d_it,
                            double* d_T, unsigned long long* d_flag);

// tbk_device_green.hip: tbk_device_green in the same way (the slabs of tbk_device_green_multi)
int tbk_device_green_slab(tbk_model* m, int64_t k_base, int axis, int layers, const double* k, int64_t nk, int M, const double* V, int64_t n_z,
                          const double* z, int max_iterations, int32_t* iterations, double* T, double* ldos, double* left, double* right, double* G,
                          double* F, double* C);

// ... and tbk_device_current (the slabs of tbk_device_current_multi)
int tbk_device_current_slab(tbk_model* m, int64_t k_base, int axis, int layers, const double* k, int64_t nk, int M, const double* V, int64_t n_z,
                            const double* z, int max_iterations, int32_t* iterations, double* T, double* ldos, double* left, double* right,
                            double* current_left, double* current_right, double* inter_left, double* inter_right, double* intra_left,
                            double* intra_right);

// roctx range around a stage (no-ops unless a roctx library can be loaded); tbk_api.hip
void tbk_range_push(const char* name);
void tbk_range_pop();

// timing scope helper: records a start/stop pair on the model stream when timing is on
struct StageTimer {
    tbk_model* m;
    EventSpan ev;
    bool on;
    hipStream_t stream;
    StageTimer(tbk_model* m_, int stage, hipStream_t s = nullptr);
    ~StageTimer();
};

// ------------------------------------------------------------------------------------------------
// kernels (each .hip file exposes plain launchers)
// ------------------------------------------------------------------------------------------------
enum HkMode { HK_TRI = 0, HK_FULL = 1 };

// One Strassen level in the dense H(k) contraction (tbk_hk_dense.hip).  Models with at least
// TBK_STRASSEN_MIN_NR padded lattice vectors are padded for it (n_r_pad a multiple of 16, ncol_pad of 128) and get the
// operand blocks d_Bs; k chunks of at least TBK_STRASSEN_MIN_NK k-points on the direct MFMA path then take it (tbk_hk_plan).
constexpr int64_t TBK_STRASSEN_MIN_NR = 1024;
constexpr int64_t TBK_STRASSEN_MIN_NK = 4096;
inline bool tbk_strassen_model(bool sparse, bool kdotp, int64_t n_r) { return !sparse && !kdotp && n_r >= TBK_STRASSEN_MIN_NR; }
inline int64_t tbk_strassen_mh(int64_t nk) { return (((nk + 1) / 2) + TBK_BM - 1) / TBK_BM * TBK_BM; }  // k rows per half
// Two levels: the table applied to each of its seven products, 49 products of quarter size.  For models whose padding gives
// whole K stages and whole element tiles in every QUARTER (k2 a multiple of 4 TBK_BK, ncol_pad of 4 TBK_BNP -- no model is padded
// further for it) and chunks of at least TBK_STRASSEN2_MIN_NK k-points; shorter chunks keep one level.  Both thresholds are the
// lower ends of the measured ranges (DESIGN_LOG.md R8.2): the deeper path won at every length tried.
constexpr int64_t TBK_STRASSEN2_MIN_NK = 8192;
inline int64_t tbk_strassen_mq(int64_t nk) { return (((nk + 3) / 4) + TBK_BM - 1) / TBK_BM * TBK_BM; }  // k rows per quarter

// How the H(k) of one chunk of k-points is computed: the contraction path and the rows it reads.  tbk_hk_plan
// (tbk_hk_dense.hip) is the only place that chooses them; the phase rows of a chunk (tbk_api.hip fill_rows) and its
// contraction (build_h) are made from the same plan.
enum HkPath {
    HK_PATH_CSR,       // sparse models (tbk_hk_csr.hip)
    HK_PATH_TINY,      // one k-point of a small model in one launch (hk_tiny_kernel)
    HK_PATH_GEMV,      // the matrix-vector kernel (hk_gemv_kernel), `splits` K slices
    HK_PATH_STRASSEN,  // one Strassen level on the MFMA tiles (launch_strassen)
    HK_PATH_STRASSEN2, // two Strassen levels (launch_strassen2)
    HK_PATH_TILES,     // the MFMA tiles, split along K `splits` ways (1: not split)
};
enum HkRows {
    HK_ROWS_NONE,      // the H(k) kernel makes them from k (d_A = NULL)
    HK_ROWS_PHASE,     // A[K2][nk_pad] cos / sin rows
    HK_ROWS_MONOMIAL,  // A[K2][nk_pad] k.p monomials
    HK_ROWS_STRASSEN,  // the seven blocks As[7][K2 / 2][Mh]
    HK_ROWS_STRASSEN2, // the 49 blocks As2[49][K2 / 4][Mq]
};
struct tbk_hk_plan_t {
    tbk_operand_t op;         // what the chunk is contracted with: its rows and its contraction are both made for it
    HkPath path = HK_PATH_TILES;
    HkRows rows = HK_ROWS_PHASE;
    int64_t nk = 0;
    int64_t nk_pad = 0;       // the row stride of A: whole k tiles
    int64_t row_doubles = 0;  // ws_phase for the rows (reserved for HK_ROWS_NONE as well)
    int splits = 1;           // GEMV: K slices; TILES: K splits
    size_t lds = 0;           // GEMV: dynamic LDS per workgroup
};
// A function of the model's options and packed columns, the operand (the staged one, or a folded one: only the staged one
// has Strassen blocks) and nk.  caller_rows: the caller makes the phase rows whatever the path (never HK_ROWS_NONE).
// classical (only with caller_rows): never a Strassen path, so that the rows are A[K2][nk_pad] whatever nk (tbk_hk_dense.hip).
tbk_hk_plan_t tbk_hk_plan(const tbk_model* m, const tbk_operand_t& op, int64_t nk, bool caller_rows, bool classical = false);
// tbk_hk_dense.hip: chunks of up to this many k-points give a k-point the same bits under a classical caller-rows plan whatever their
// length (INT64_MAX: any; 0: the model is too large for that -- tbk_optics.hip caps its walk with it)
int64_t tbk_hk_stable_chunk(const tbk_model* m);

// ONE k-point on host buffers (tbk_hamilton / tbk_eigenval) whose plan is HK_ROWS_NONE: k goes into the kernel arguments (no
// upload) and the H(k) kernel forms the convention-1 phases itself from the raw positions.  Those two entry points decide
// and pass this down; tbk_launch_hk_dense consumes it and refuses it for any other plan.  Default-constructed: not such a call.
struct tbk_one_k_t {
    const double* h_k = nullptr;        // the caller's k-point [dim] on the host, read while the launch is made
    const double* d_pos_raw = nullptr;  // convention 1: the raw positions [n_orb][dim] on the device (tbk_model::ws_posraw)
};

// tbk_api.hip: k-points per chunk (with_eig: room for the eigensolver's buffers too), and H(k) of one chunk for its plan:
// chunk_h is fill_rows (the phase rows, in ws_phase), then, for convention 1, the chunk's orbital phases from d_pos_raw (in
// ws_orb) unless one_k brings the k-point, then the contraction.  Only the pipeline in tbk_api.hip enqueues the rows apart.
int64_t choose_chunk(tbk_model* m, int64_t nk, bool with_eig);
int fill_rows(tbk_model* m, const tbk_hk_plan_t& plan, const double* d_k);
int chunk_h(tbk_model* m, const tbk_hk_plan_t& plan, int mode, int convention, const double* d_k, const double* d_pos_raw,
            const tbk_one_k_t& one_k, double* d_H);
// D^a = (1 / 2 pi) dH/dk_a of nk k-points, FULL, convention 2, in pieces of choose_chunk: the derivative rows (tbk_phase.hip) in
// ws_phase, then the contraction of a classical caller-rows plan with the staged operand (tbk_optics.hip; tbk_hamilton_derivative_device)
int tbk_chunk_dh(tbk_model* m, int axis, const double* d_k, int64_t nk, double* d_D);

// tbk_api.hip: tbk_eigenval_device_hint with a hook (NULL: none).  The chunk pipeline calls it whenever the eigenvalues of rows
// [c0, c0 + nkc) of the call have been enqueued, with an event recorded behind them (tbk_comm.hip); the rocSOLVER path never does.
using tbk_chunk_hook_t = std::function<int(int64_t c0, int64_t nkc, hipEvent_t done)>;
int tbk_eigenval_device_hooked(tbk_model* m, const double* d_k, const double* h_k, int64_t nk, double* d_E, const tbk_chunk_hook_t* on_chunk);

// tbk_phase.hip
int tbk_launch_phase_strassen(tbk_model* m, const tbk_operand_t& op, const double* d_k, int64_t nk, double* d_As);
int tbk_launch_phase_strassen2(tbk_model* m, const tbk_operand_t& op, const double* d_k, int64_t nk, double* d_As2);
int tbk_launch_phase(tbk_model* m, const tbk_operand_t& op, const double* d_k, int64_t nk, int64_t nk_pad, double* d_A);
int tbk_launch_phase_derivative(tbk_model* m, const tbk_operand_t& op, const double* d_k, int64_t nk, int64_t nk_pad, int axis, double* d_A);
int tbk_launch_orbital_phases(tbk_model* m, const double* d_k, const double* d_pos, int64_t nk, double* d_orb);
int tbk_launch_monomials(hipStream_t s, const int32_t* d_powers, int dim, int64_t n_p,
                         int64_t n_p_pad, const double* d_k, int64_t nk, int64_t nk_pad,
                         double* d_A);

// tbk_stage.hip
int tbk_stage_dense(tbk_model* m, const double* d_hop_raw);
int tbk_stage_kdotp(tbk_model* m, const double* d_coeff_raw);
int tbk_stage_strassen(tbk_model* m);
size_t tbk_strassen2_bytes(const tbk_model* m);
int tbk_stage_strassen2(tbk_model* m);  // builds d_Bs2 from d_Bs if it is missing

// tbk_hk_dense.hip: the H(k) of plan.nk k-points with plan.op along plan.path (not HK_PATH_CSR); d_A holds the plan's rows
int tbk_launch_hk_dense(tbk_model* m, const tbk_hk_plan_t& plan, const double* d_A, int mode, int convention,
                        const double* d_k, const double* d_pos, const tbk_one_k_t& one_k, double* d_H);

// ... and of n_lines mesh lines in one launch: line t takes the operand b_stride doubles behind that of line t - 1 (op: line 0)
int tbk_launch_hk_dense_lines(tbk_model* m, const tbk_operand_t& op, const double* d_A, int64_t n_lines, int line_len, int64_t b_stride,
                              double* d_H);

// tbk_hk_csr.hip
int tbk_launch_hk_csr(tbk_model* m, const double* d_A, int64_t nk, int64_t nk_pad, int mode,
                      int convention, const double* d_k, const double* d_pos, double* d_H);

// host side of the sparse path: k-points per LDS phase tile for n_r lattice vectors (0: the tile does not fit), and the
// conflict-free walk order of the per-element records for that tile shape
int tbk_csr_tile_kpoints(int64_t n_r);
void tbk_csr_schedule(int ncol, int kt, const std::vector<int64_t>& cptr, const std::vector<int32_t>& rec_r, const std::vector<double>& rec_v,
                      std::vector<int64_t>& sptr, std::vector<int32_t>& srec_r, std::vector<double>& srec_v);

// tbk_eig.hip
int tbk_eig_batched(tbk_model* m, double* d_H, int64_t nk, double* d_E);    // full rocSOLVER zheevd

// tbk_eigh.hip: the checks of the eigh entry points that need no model (convention, pos, nk)
int tbk_eigh_check_arguments(int64_t nk, int convention, const double* pos);
// tbk_eigh_device with the choice of how H(k) is built: caller_rows = true keeps every chunk on the paths that read finished phase
// rows (tbk_hk_plan's caller_rows and classical), whatever its length -- tbk_optics.hip, whose sums must not know the chunk
int tbk_eigh_device_rows(tbk_model* m, const double* d_k, int64_t nk, int convention, const double* d_pos, double* d_E, double* d_U,
                         bool caller_rows);

// ------------------------------------------------------------------------------------------------
// The eigensolver's plan (tbk_eig_plan.hip).  How the matrices of one eigenvalue CALL are reduced and solved: tbk_eig_plan is
// the only place that chooses, the entry points make the plan once and every launcher picks its instantiation from its fields.
// A function of the orbital count, the model's `eigensolver` option, the k-points of the call, the requested method (tbk.h:
// TBK_REDUCE_AUTO is what eigenval takes) and the environment switches, of nothing else.  Of the CALL, never of a chunk: several
// of the variants differ in the last bit, and TBK_OPT_K_CHUNK must not change a result (tests/test_gpu_parity.py).
// ------------------------------------------------------------------------------------------------
constexpr int ST_MAXN = 512;              // the one-stage streaming kernel (tbk_eig_stream.hip): 64 < n <= 512
constexpr int BAND_ONE_WG_MAXN = 1024;    // one workgroup per matrix: two rows per thread of 512 threads, X (8 complex per row) is 128 KiB of LDS
constexpr int BAND_LDS_CHASE_MAXN = 512;  // above: the chase keeps its 16 diagonals in global memory
// own kernels or not: rocSOLVER (TBK_EIG_ROCSOLVER, or a size / method they do not cover), register-resident (n <= 64,
// tbk_eig_small.hip), one-stage streaming (tbk_eig_stream.hip), two-stage dense -> band -> tridiagonal (tbk_eig_band*.hip)
enum EigFamily { EIG_ROCSOLVER, EIG_REGISTER, EIG_ONE_STAGE, EIG_TWO_STAGE };
// the second stage's 16 working diagonals: in LDS (band_chase4_kernel), in a cyclic LDS window of 272 columns / 16 sweep slots or
// of 512 columns / 32 slots (band_chase4w_kernel), in global memory (band_chase4g_kernel)
enum EigChase { EIG_CHASE_LDS, EIG_CHASE_WINDOW16, EIG_CHASE_WINDOW32, EIG_CHASE_GLOBAL };
struct tbk_eig_plan_t {
    int n = 0;                   // orbitals
    int64_t call_nk = 0;         // k-points of the call
    EigFamily family = EIG_ROCSOLVER;
    bool split_on = false;       // register kernels (also the 64 x 64 tail of one-stage): the trailing 32 x 32 block as a second launch
    bool reg128 = false;         // one-stage, 65 - 128 orbitals: the 128-row register kernel instead of the streaming one
    bool via128 = false;         // one-stage above 128: the streaming kernel hands over at the trailing 128 x 128 block (else 64 x 64)
    bool reg128_nw2 = false;     // the 128-row register kernel on four waves up to 96 rows (else eight at every size)
    bool chain = false;          // first stage: the launch chain of band_xl_* (else one workgroup per matrix)
    bool chain_by_size = false;  // ... at every call size (above TBK_BAND_XL_FROM orbitals): batches go in groups, tbk_eig_xl_groups
    bool wide = false;           // one workgroup per matrix: its eight-wave, row-per-thread form
    bool fused = false;          // second stage: inside the first-stage kernel (else a launch of its own)
    EigChase chase = EIG_CHASE_LDS;
    bool chase_buffer = false;   // a matrix' band buffer carries the 16 working diagonals behind the compact band
    bool bisect = false;         // tridiagonal stage: bisection (else the lane-per-matrix QL)
    int bisect_lanes = 1;        // lanes per eigenvalue of the bisection kernel
    // bytes per matrix of the workspaces (0: the path does not use them); band_stride: bytes between the matrices of a band buffer
    size_t band_stride = 0, ws_band = 0, ws_bandmat = 0, ws_xl = 0;
    bool own() const { return family != EIG_ROCSOLVER; }
};
tbk_eig_plan_t tbk_eig_plan(int n_orb, int eigensolver, int64_t call_nk, int method = TBK_REDUCE_AUTO);
int tbk_eig_check_option(const tbk_model* m);  // TBK_EIG_WAVE is the register-resident kernels: an error above 64 orbitals
// the range checks of the argument validation: 1 .. 64; 65 .. 4096 (1024 with TBK_BAND_XL=0: the two-stage kernels cover all of it)
bool tbk_eig_small_supported(int n);
bool tbk_eig_band_supported(int n);
// What depends on one LAUNCH, not on the call, takes the plan and keeps the chunk length out of it: the groups a launch of nk
// matrices above TBK_BAND_XL_FROM orbitals goes in (per matrix the same launches in the same order, the same bits).  The others
// are arguments in tbk_api.hip: `beside_ql`, "the last chunk of a pipeline bisects", and tbk_eig_reduce's d_band (the second
// stage of a chunk goes to the tridiagonal stream: that needs a following chunk).
int tbk_eig_xl_groups(const tbk_eig_plan_t& plan, int64_t nk);
size_t tbk_eig_scratch_per_k(const tbk_model* m);
// ws_band / ws_xl for launches of up to max_nk matrices and `bandmats` of the ws_bandmat (one per chunk in flight), from the
// plan's byte counts.  In front of the pipeline, never inside a launch (tbk_eig_band_xl.hip)
int tbk_eig_reserve(tbk_model* m, const tbk_eig_plan_t& plan, int64_t max_nk, int bandmats);
// Reduce nk matrices on stream s per the plan: d_H (upper triangle of the row-major H) is overwritten, d_de receives d[nk][n]
// followed by e[nk][n].  d_band != NULL (two-stage, second stage a launch of its own): the first stage alone, the band goes
// there and the caller runs tbk_launch_band_chase; else both stages in order on s.
int tbk_eig_reduce(tbk_model* m, const tbk_eig_plan_t& plan, hipStream_t s, double* d_H, int64_t nk, double* d_de, void* d_band = nullptr);

// tbk_eig_stream.hip: the one-stage reduction (64 < n <= 512) and the bisection
int tbk_launch_tridiag_stream(tbk_model* m, const tbk_eig_plan_t& plan, hipStream_t s, double* d_H, int64_t nk, double* d_de);
int tbk_launch_bisect(tbk_model* m, const tbk_eig_plan_t& plan, hipStream_t s, const double* d_de, int64_t nk, double* d_E);

// tbk_eig_band.hip: two-stage reduction (dense -> band on the matrix pipe, band -> tridiagonal in LDS)
size_t tbk_band_scratch_per_matrix(int n);
size_t tbk_band_bytes_per_matrix(int n, bool chase_buffer);
// d_de_fused != NULL: every workgroup runs the second stage for its matrix too and writes (d, e); d_band is not used.  (A plan
// on the launch chain: the second stage of every group behind its first stage; d_band is used.)
int tbk_launch_band_reduce(tbk_model* m, const tbk_eig_plan_t& plan, hipStream_t s, double* d_H, int64_t nk, void* d_vw, void* d_band,
                           double* d_de_fused = nullptr);
int tbk_launch_band_chase(tbk_model* m, const tbk_eig_plan_t& plan, hipStream_t s, const void* d_band, int64_t nk, double* d_de);

// tbk_eig_small.hip
// (above 32 orbitals the head of every matrix in d_H is overwritten with its trailing 32 x 32 block: H is consumed)
int tbk_launch_tridiag(tbk_model* m, const tbk_eig_plan_t& plan, hipStream_t s, double* d_H, int64_t nk, double* d_de);
// 64 < n <= 128: the eight-wave register kernel does the first n - 64 steps
int tbk_launch_tridiag_reg128(const tbk_eig_plan_t& plan, hipStream_t s, double* d_H, int n, int64_t nk, double* d_D, double* d_E, int64_t h_stride, int ldd, int off);
int tbk_launch_tridiag_tail64(const tbk_eig_plan_t& plan, hipStream_t s, double* d_H, int64_t nk, double* d_D, double* d_E, int n_full);  // tbk_eig_stream.hip hands over here
// `beside_ql`: this launch shares the chip with another QL launch (the tail of the chunk pipeline): use
// half-size workgroups (32 KiB of LDS) that fit next to two resident 64 KiB ones.
int tbk_launch_ql(tbk_model* m, hipStream_t s, const double* d_de, int64_t nk, double* d_E, bool beside_ql = false);

// tbk_fold.hip
// Chunks of a folded call: whole runs (mesh planes) packed up to the chunk size
std::vector<int64_t> run_schedule(const std::vector<int64_t>& runs, int64_t chunk);

// The mesh lines of a piece [lo, hi) of one run (tbk_fold.hip: analyse)
struct LineInfo {
    bool ok = false;     // the piece has a body of whole mesh lines
    int e2 = -1;         // reduced component shared along a line
    int64_t L = 0;       // points per line
    int64_t body = 0;    // first point of the body
    int64_t n_lines = 0;
};

// One eigenvalue call on a k list with long runs of one shared component (grids in meshgrid order, stacks of planes): every
// run is evaluated with the operand folded along that component.  The chunk pipeline (tbk_api.hip) runs over the whole list
// and calls build() for the H(k) of every chunk, which is assembled run by run.
struct tbk_folded_call {
    // h_k: the caller's host copy of the list, or NULL.  Device-resident lists are never read back (include/tbk.h: the device
    // entry points enqueue and return): the run structure comes from that copy (tbk_eigenval / tbk_eigenval_device_hint) or
    // not at all.
    tbk_folded_call(tbk_model* m, const double* d_k, const double* h_k, int64_t nk);
    bool folds() const { return f >= 0; }  // else the call takes the direct path
    std::vector<int64_t> runs;             // first k-point of every run, and nk
    int begin();                           // the k-points without the folded component (main stream), in front of the first build()
    int build(int64_t c0, int64_t nkc, double* d_H);  // H of k-points [c0, c0 + nkc) of the call (main stream)

private:
    int run_operand(size_t r, tbk_operand_t* op);
    int piece_plane(const tbk_operand_t& op, int64_t lo, int64_t hi, double* d_Hp);
    int fold_body(const tbk_operand_t& from, tbk_fold_plan_t& plan2, const LineInfo& li, int64_t a0, int64_t n, int slot0);
    int contract_lines(tbk_fold_plan_t& plan2, const LineInfo& li, int64_t a0, int64_t n, double* d_Hp);
    int piece(const tbk_operand_t& op, int64_t lo, int64_t hi, double* d_Hp);
    int batched(int64_t c0, int64_t nkc, double* d_H, bool* done);

    tbk_model* m;
    const double* d_k;
    const double* h_k;
    int64_t nk;
    int f = -1;                       // the folded component (-1: the list does not fold)
    int dim = 0, dim1 = 0;            // of the model, of a folded run
    size_t nn2 = 0;                   // doubles per H(k)
    tbk_fold_plan_t* plan1 = nullptr; // folds the staged operand along f
    std::vector<int> reduced;         // original component of every reduced one
    int64_t group_lo = -1;            // first run of the group whose operands are in plan1's buffer
    double* d_k2 = nullptr;           // [nk][dim1] the k-points without component f (ws_kfold)
};

// tbk_dos.hip: the share of cells [p_lo, p_lo + p_count) along axis 0 of a mesh in nos (tbk_dos is the whole axis; tbk_dos_multi
// gives every handle one slab)
int tbk_dos_slab(tbk_model* m, const int32_t* mesh, int64_t p_lo, int64_t p_count, double e_min, double e_step, int64_t n_e, double* nos_out);

// tbk_pdos.hip: the same for the projected number of states (nos_out[n_groups][n_e]), and the check of the groups
int tbk_pdos_check_groups(int n_orb, const int32_t* group_offsets, const int32_t* group_orbitals, int n_groups);
int tbk_pdos_slab(tbk_model* m, const int32_t* mesh, int64_t p_lo, int64_t p_count, const int32_t* group_offsets, const int32_t* group_orbitals,
                  int n_groups, double e_min, double e_step, int64_t n_e, double* nos_out);
// ... its plan and launch for weights the caller made itself (tbk_tdf.hip): W[nk][n_groups][n_orb] in [0, 1]
int tbk_pdos_weighted_bytes(int dim, const int32_t* mesh, int64_t cells0, int64_t planes0, int n_orb, int n_groups, int64_t n_e, size_t* ws_bytes);
int tbk_pdos_weighted_launch(hipStream_t s, int dim, const int32_t* mesh, int64_t cells0, int64_t planes0, int n_orb, int n_groups, int64_t n_e,
                             const double* d_E, const double* d_W, double e_min, double e_step, double denom, void* d_ws, double* d_nos,
                             SpanRecorder& timer);

// tbk_tdf.hip: the checks that need no device, and one handle's part of a call: the whole call (cumulative_out[G][n_e]), or for a call
// on several handles E and W of the planes [p_lo, p_lo + p_count) of axis 0 to the host, or the accumulation of the whole mesh from there
enum { TBK_TDF_WHOLE = 0, TBK_TDF_WEIGHTS = 1, TBK_TDF_ACCUMULATE = 2 };
int tbk_tdf_check_arguments(int dim, double degeneracy, const double* scale);
int tbk_tdf_slab(tbk_model* m, const int32_t* mesh, int64_t p_lo, int64_t p_count, double e_min, double e_step, int64_t n_e, double degeneracy,
                 const double* scale, int mode, double* h_E, double* h_W, double* cumulative_out);

// tbk_peak.hip
int tbk_run_mfma_f64_peak(double* tflops);
