/*
 * tbk.h -- C ABI of libtbk.so: the MI355X (gfx950) k-space evaluation path of a tight-binding model.
 *
 *     H(k) = sum_R exp(2 pi i k.R) hop[R]  +  h.c.        and        eigenvalues of H(k)
 *
 * The reference (Z2PackDev/TBmodels 1.4.4) is pure Python and has NO FFI / plugin interface for
 * this path: the path is two bound methods of tbmodels.Model.  This header is therefore the
 * boundary a maintainer would bind (ctypes stub in INTEGRATION.md) to replace the bodies of
 *
 *     Model.hamilton(k, convention=2)   /root/reference/src/tbmodels/_tb_model.py:1076-1132
 *     Model.eigenval(k)                 /root/reference/src/tbmodels/_tb_model.py:1134-1150
 *     KdotpModel.hamilton / eigenval    /root/reference/src/tbmodels/kdotp.py:51-100
 *
 * Conventions
 *   - plain pointers and sizes only; complex128 is passed as interleaved (re, im) doubles;
 *   - every array is C-contiguous, row-major, in the reference's own layouts:
 *       R    int32   [n_r][dim]          lattice vectors = keys of model.hop (_tb_model.py:206-210)
 *       hop  double  [n_r][n_orb][n_orb][2]   = values of model.hop: half-space blocks, the R = 0
 *                                             block stored HALVED (_tb_model.py:268, :218)
 *       k    double  [nk][dim]           reduced coordinates, NOT reduced mod 1 (_tb_model.py:1103-1108)
 *       pos  double  [n_orb][dim]        orbital positions, only read for convention 1 (:1124-1128)
 *       H    double  [nk][n_orb][n_orb][2]    H[k][i][j] (_tb_model.py:1109)
 *       E    double  [nk][n_orb]         ascending eigenvalues per k (scipy.linalg.eigvalsh, :1149)
 *   - every function returns 0 on success, a tbk_status otherwise; tbk_last_error() gives the
 *     message of the calling thread's last failure;
 *   - "host" entry points take caller-owned host memory and return when the result is in it;
 *     "device" entry points take device pointers on the model's device, enqueue on the model's
 *     streams and return without synchronising and without reading device memory back
 *     (tbk_synchronize waits);
 *   - a handle's staged model is immutable after creation (re-create it when model.hop changes);
 *     host threads calling into ONE handle are serialised by a lock inside it (they share its
 *     workspaces and streams); different handles are independent and run concurrently.
 *
 * There is no CPU implementation behind this interface: without a gfx950 device every compute
 * entry point fails with TBK_ERR_DEVICE.
 */
#ifndef TBK_H
#define TBK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tbk_model tbk_model; /* staged hoppings + workspaces on one device */
typedef struct tbk_kdotp tbk_kdotp; /* staged Taylor coefficients of a k.p model   */
typedef struct tbk_comm tbk_comm;   /* RCCL communicator of one rank               */

typedef enum tbk_status {
    TBK_OK = 0,
    TBK_ERR_ARGUMENT = 1, /* bad size / null pointer / convention not in {1, 2}  -> ValueError   */
    TBK_ERR_DEVICE = 2,   /* no device, HIP / rocBLAS / RCCL failure              -> RuntimeError */
    TBK_ERR_MEMORY = 3,   /* device allocation failed                             -> MemoryError  */
    TBK_ERR_NOT_FINITE = 4, /* NaN / Inf in H(k): scipy check_finite=True         -> ValueError   */
    TBK_ERR_NO_CONVERGENCE = 5, /* eigensolver / decimation did not converge      -> LinAlgError  */
    TBK_ERR_SINGULAR = 6  /* tbk_green_dressed: z - H(k) - Sigma(z) is singular; tbk_surface_green: z - e is; tbk_transmission: z - D_p is -> LinAlgError  */
} tbk_status;

/* eigensolver selection for tbk_model_set_option(TBK_OPT_EIGENSOLVER, ...):
 *   WAVE      hand-written register-resident Householder reduction (n_orb <= 64 only) + tridiagonal stage
 *   ROCSOLVER rocsolver_zheevd_strided_batched
 *   AUTO      WAVE when n_orb <= 64; the own one- / two-stage Householder kernels up to n_orb = 4096 (above 1024 orbitals the
 *             first stage is a chain of launches per panel, csrc/tbk_eig_band.hip band_xl_*); ROCSOLVER above.
 * Tridiagonal stage of the two hand-written paths: lane-per-matrix QL for large batches of n_orb <= 64,
 * bisection on Sturm counts otherwise (n_orb > 64, calls of <= max(4096, 768 n_orb) k-points, and the last
 * chunk of a call).  Both are backward stable; they agree to rounding, so eigenvalues are reproducible run to
 * run but depend on the batch size at the 1e-13 level.  The same holds for the reduction above 128 orbitals: calls of
 * a few matrices take wider kernels / a chain of launches (tbk_eig_plan.hip: the plan's `chain`, `wide`) whose partial sums
 * differ from the one-workgroup kernels' in the last bit.  Bitwise reproducibility is therefore a property of a CALL SHAPE:
 * the same k list on the same number of devices / ranks (tbk_eigenval_multi and ShardedEigenval cut it into
 * ceil(nk / n) slabs, and every slab chooses its kernels by ITS size) gives the same bits every time; the same list on a
 * different device count agrees to rounding only. */
enum { TBK_EIG_AUTO = 0, TBK_EIG_WAVE = 1, TBK_EIG_ROCSOLVER = 2 };
enum {
    TBK_OPT_EIGENSOLVER = 1, /* one of TBK_EIG_*                                           */
    TBK_OPT_K_CHUNK = 2,     /* max k-points per internal chunk (0 = choose from free HBM) */
    TBK_OPT_TIMING = 3,      /* 1: bracket every kernel with HIP events (tbk_get_timing)   */
    TBK_OPT_FOLD = 4,        /* 0: never fold k lists with long runs of one shared component (grids) into
                              *    lower-dimensional models (default 1; dense models, eigenval only)          */
    TBK_OPT_STRASSEN = 5,    /* 0: dense H(k) of long k chunks as the classical product instead of Strassen's
                              *    (default 1; csrc/tbk_hk_dense.hip tbk_hk_plan)                              */
    TBK_OPT_STRASSEN_LEVELS = 6, /* 1 or 2 (default 2): the deepest recursion a chunk may take while TBK_OPT_STRASSEN
                              *    is on -- two levels need longer chunks than one (tbk_hk_plan); anything else is
                              *    TBK_ERR_ARGUMENT                                                            */
    TBK_OPT_STRASSEN_COMBINE = 7 /* 1 (default): the combine of a two-level chunk of the eigenvalue path in two passes,
                              *    the first beside the last products (launch_strassen2); 0: the single kernel behind
                              *    them.  Same bits either way                                                 */
};

/* ---- library / device ------------------------------------------------------------------ */
const char* tbk_version(void);
const char* tbk_last_error(void);
int tbk_device_count(int* count);

/* ---- model staging (replaces the per-call walk over model.hop, _tb_model.py:1111) ------- */

/* Dense hoppings.  `hop` = the n_r stored (n_orb x n_orb) complex blocks, in the order of `R`. */
int tbk_model_create_dense(int device, int dim, int n_orb, int64_t n_r, const int32_t* R,
                           const double* hop, tbk_model** out);

/* Sparse hoppings (model._sparse, _sparse_matrix.py:35-37): the per-R scipy CSR matrices
 * concatenated as COO triplets; entries of lattice vector r are [r_ptr[r], r_ptr[r+1]).
 * Duplicate (row, col) entries inside one R are summed, like scipy's toarray(). */
int tbk_model_create_csr(int device, int dim, int n_orb, int64_t n_r, const int32_t* R,
                         const int64_t* r_ptr, const int32_t* row, const int32_t* col,
                         const double* val, tbk_model** out);

void tbk_model_destroy(tbk_model* m);
int tbk_model_set_option(tbk_model* m, int option, int64_t value);
int tbk_model_info(const tbk_model* m, int* device, int* dim, int* n_orb, int64_t* n_r,
                   int* is_sparse, int64_t* staged_bytes);
/* Event counters of a handle since its creation (which path the eigenvalue calls took). */
enum { TBK_CNT_EIGENVAL_CALLS = 0, TBK_CNT_FOLDED_CALLS = 1, TBK_CNT_FOLDED_KPOINTS = 2,
       TBK_CNT_LIBRARY_CALLS = 3, /* eigenvalue calls handed to rocSOLVER (on request, or above the own kernels' range) */
       TBK_CNT_STRASSEN_LAUNCHES = 4, /* dense H(k) launches of a k chunk that took the Strassen product, either depth */
       TBK_CNT_STRASSEN2_LAUNCHES = 5, /* ... those of them that took two levels */
       TBK_CNT_STRASSEN2_SPLIT = 6, /* ... those of them whose combine ran in two passes (TBK_OPT_STRASSEN_COMBINE) */
       TBK_CNT_COUNT = 7 };
int tbk_model_counter(tbk_model* m, int counter, int64_t* value);

/* ---- the hot path, host buffers (what Model.hamilton / Model.eigenval call) -------------- */

/* H(k) for nk k-points.  convention in {1, 2}; pos may be NULL for convention 2. */
int tbk_hamilton(tbk_model* m, const double* k, int64_t nk, int convention, const double* pos,
                 double* H_out);

/* Ascending eigenvalues of H(k) (convention 2) for nk k-points. */
int tbk_eigenval(tbk_model* m, const double* k, int64_t nk, double* E_out);

/* Eigenvalues AND eigenvectors of H(k) in `convention` (1 or 2; pos as for tbk_hamilton; Model.eigh):
 *   E  double [nk][n_orb]             ascending eigenvalues per k
 *   U  double [nk][n_orb][n_orb][2]   U[k][i][j] = component i of the unit eigenvector of E[k][j] (columns, as in
 *                                     scipy.linalg.eigh); the columns of every U[k] are orthonormal
 * The phase of every column, and the basis inside a degenerate eigenspace, are unspecified (as in LAPACK).
 * n_orb <= 64 (TBK_EIG_AUTO / _WAVE): parallel cyclic Jacobi in LDS (csrc/tbk_eigh.hip), whose result for one matrix does not
 * depend on the call shape; above 64 orbitals or with TBK_EIG_ROCSOLVER: rocsolver_zheev_strided_batched
 * (TBK_CNT_LIBRARY_CALLS); TBK_EIG_WAVE above 64 orbitals is TBK_ERR_ARGUMENT.  Non-finite H(k) -> TBK_ERR_NOT_FINITE
 * (NaN rows in E and U), no convergence -> TBK_ERR_NO_CONVERGENCE.  The solver's time is charged to TBK_T_EIG. */
int tbk_eigh(tbk_model* m, const double* k, int64_t nk, int convention, const double* pos, double* E_out, double* U_out);

/* ---- the hot path on several devices from ONE process (host buffers) ----------------------
 * handles[0..n_handles) are staged copies of the SAME model, normally one per device (several on one device are
 * allowed).  The k list is cut into contiguous slabs of ceil(nk / n_handles) rows (handle i takes slab i; the last
 * slabs may be short or empty), every slab runs on its handle's device from its own host thread, and every device
 * copies its result straight into its rows of the caller's array: k-points are independent (_tb_model.py:1111-1123)
 * and the result is in caller order (:1147-1150) without any exchange.  Mesh slabs are folded like whole meshes.
 * On failure the status and message of the first failing slab in k order are returned (a NaN k-point gives
 * TBK_ERR_NOT_FINITE exactly once).  n_handles == 1 is tbk_eigenval / tbk_hamilton. */
int tbk_eigenval_multi(tbk_model* const* handles, int n_handles, const double* k, int64_t nk, double* E_out);
int tbk_hamilton_multi(tbk_model* const* handles, int n_handles, const double* k, int64_t nk, int convention,
                       const double* pos, double* H_out);
int tbk_eigh_multi(tbk_model* const* handles, int n_handles, const double* k, int64_t nk, int convention,
                   const double* pos, double* E_out, double* U_out);

/* ---- the hot path, device buffers (bench, sharded runs, device-side consumers) ----------- */
int tbk_hamilton_device(tbk_model* m, const double* d_k, int64_t nk, int convention,
                        const double* d_pos, double* d_H);
int tbk_eigenval_device(tbk_model* m, const double* d_k, int64_t nk, double* d_E);
/* tbk_eigh on device buffers: H(k) of every chunk is built straight into its rows of d_U and overwritten there by its
 * eigenvectors (no N^2 workspace).  Enqueued only: the non-finite / convergence flags are reported by tbk_eigenval_check. */
int tbk_eigh_device(tbk_model* m, const double* d_k, int64_t nk, int convention, const double* d_pos, double* d_E,
                    double* d_U);
/* The same for a caller that still holds the host array it uploaded: h_k == the contents of d_k (or NULL).
 * Device-resident lists are never read back -- that would synchronise -- so long runs of one shared k component
 * (uniform meshes in meshgrid order, stacks of planes; TBK_OPT_FOLD) are only recognised through h_k: the run
 * STRUCTURE and the shared-component values are taken from h_k, everything else from d_k.  tbk_eigenval_device is
 * this call with h_k = NULL (never folds); tbk_eigenval (host buffers) always has the list. */
int tbk_eigenval_device_hint(tbk_model* m, const double* d_k, const double* h_k, int64_t nk, double* d_E);
/* The k chunks a tbk_eigenval_device call of nk k-points on this model would run as now (TBK_OPT_K_CHUNK, the free device
 * memory and the contraction path of the last chunk enter; folded calls cut whole runs instead): *n_chunks of them, the first
 * min(*n_chunks, capacity) lengths in lengths[].  Read-only, enqueues nothing; TBK_ERR_ARGUMENT for models whose eigenvalue
 * calls go to rocSOLVER. */
int tbk_eigenval_schedule(tbk_model* m, int64_t nk, int64_t* lengths, int capacity, int* n_chunks);
/* Check the info flags of the eigenvalue calls since the last check (synchronises). */
int tbk_eigenval_check(tbk_model* m);
int tbk_synchronize(tbk_model* m);

/* ---- the eigensolver's reduction stage alone (scipy.linalg.eigvalsh of _tb_model.py:1149 = this + the tridiagonal stage)
 * nk Hermitian matrices H[nk][n_orb][n_orb][2] (row-major; only the upper triangle i <= j is read) are reduced to real
 * symmetric tridiagonal form with the same eigenvalues: d[nk][n_orb] diagonals, e[nk][n_orb] off-diagonals (e[.][n-1] = 0).
 * n_orb <= 4096.  method: TBK_REDUCE_AUTO = what tbk_eigenval takes for this size (register-resident reduction up to 64
 * orbitals, one-stage reduction up to 188 -- in registers up to 128, streaming above -- two-stage reduction -- dense ->
 * band of half-width 8 on the matrix pipe, band -> tridiagonal by bulge chasing -- from 185 to 4096); _ONE_STAGE / _TWO_STAGE force one of them (one-stage:
 * n_orb <= 512 only; two-stage: 64 < n_orb <= 4096 only).  H_reduced (may be NULL) receives the work copy of the matrices as the reduction left it:
 * after the two-stage reduction its upper triangle holds the band form of stage one.
 * Host buffers; synchronous.  For tests and for callers that bring their own matrices. */
enum { TBK_REDUCE_AUTO = 0, TBK_REDUCE_ONE_STAGE = 1, TBK_REDUCE_TWO_STAGE = 2 };
int tbk_tridiagonal_reduce(int device, int n_orb, int64_t nk, const double* H, int method, double* d, double* e,
                           double* H_reduced);

/* The reduction stage alone on the chip, timed with HIP events on random Hermitian matrices made on the device (nothing
 * crosses PCIe): us_per_matrix[0] = the reduction as tbk_eigenval runs it for this size and call size (both stages of the
 * two-stage path), [1] = its first stage (dense -> band) alone, [2] = its second stage (band -> tridiagonal) alone -- [1],
 * [2] are 0 below the two-stage sizes.  Mean over `reps` repetitions after one warm-up.  Measurement only (bench.py
 * `eig_roofline.standalone`): the in-pipeline stage time shares the FP64 pipe with the next chunk's H(k). */
int tbk_reduce_standalone(int device, int n_orb, int64_t nk, int reps, double* us_per_matrix);

/* ---- density of states of a uniform k mesh: the linear tetrahedron method (not in the reference) ---------------------------
 * mesh   int32 [dim]   a Gamma-centred, periodic mesh: k = (i_1 / n_1, ..., i_dim / n_dim) in np.meshgrid(indexing="ij") order
 * the energy grid is E_j = e_min + j e_step, j = 0 .. n_e - 1  (2 <= n_e <= 2^20, e_step > 0)
 * nos    double [n_e]  nos[j] = states per unit cell with energy <= E_j, from linear interpolation of every band inside the six
 *                      tetrahedra that share the main diagonal of a mesh cell (dim = 3; its two triangles in dim = 2).  The density
 *                      of states is its difference quotient; nos[n_e - 1] == n_orb when the grid ends above the spectrum.
 * Only dim in {2, 3}.  The kernel (csrc/tbk_dos.hip) accumulates in 64-bit fixed point with a resolution of 2^-40 per simplex
 * (|error| <= 4.5e-13 n_orb) and sums in integers, so for given eigenvalues nos does not depend on the order in which the
 * device runs its waves: the same call gives the same bits, as for the eigenvalues above.
 * Range: the kernels (this one and tbk_pdos) work on energies multiplied by 2^54, so that a corner gap down to the smallest
 * subnormal has a finite reciprocal; eigenvalues and grid points must stay below 2^969 in magnitude (not checked).
 * Argument errors (TBK_ERR_ARGUMENT): dim not in {2, 3}, a mesh entry < 1, 2^31 mesh points or more, n_e outside [2, 2^20],
 * e_step <= 0 or not finite, e_min not finite, a NULL pointer, a k.p handle.  Host buffers; synchronous. */

/* The kernel alone on eigenvalues the caller brings: E[NK][n_orb] in mesh order, every row ascending (what tbk_tridiagonal_reduce is
 * to the eigensolver: for tests, and for callers that have their own eigenvalues). */
int tbk_dos_from_eigenvalues(int device, int dim, const int32_t* mesh, int n_orb, const double* E, double e_min, double e_step,
                             int64_t n_e, double* nos_out);
/* The whole call: the mesh's k list is made on the host and evaluated through the path of tbk_eigenval_device_hint (dense models
 * fold, CSR models work unchanged), the eigenvalues of the whole mesh stay in device memory (NK n_orb doubles; TBK_ERR_MEMORY
 * when they do not fit), the kernel runs on them and n_e doubles come back.  Non-finite eigenvalues and no convergence are
 * reported as by tbk_eigenval, in front of the kernel. */
int tbk_dos(tbk_model* m, const int32_t* mesh, double e_min, double e_step, int64_t n_e, double* nos_out);
/* On several devices from one process (handles as for tbk_eigenval_multi): handle i takes a contiguous slab of ceil(n_1 / n_handles)
 * cells along axis 0 and evaluates its planes plus the one periodic neighbour plane it needs; the host adds the handles' shares in
 * handle order; handles whose slab is empty are skipped.  n_handles == 1 is tbk_dos.  The internal eigenvalue calls have another
 * shape than on one device, so the result agrees with tbk_dos to rounding (1e-13 level), not bitwise. */
int tbk_dos_multi(tbk_model* const* handles, int n_handles, const int32_t* mesh, double e_min, double e_step, int64_t n_e,
                  double* nos_out);
/* While TBK_OPT_TIMING is on: ms = summed HIP-event time of the density-of-states kernels of this handle's tbk_dos calls (the
 * eigenvalue stages are in tbk_get_timing, whose array length is fixed), calls = how many; reset = 1 clears. */
int tbk_dos_timing(tbk_model* m, double* ms, int64_t* calls, int reset);

/* ---- orbital-projected density of states of a uniform k mesh (not in the reference) ------------------------------------------
 * The linear tetrahedron method with matrix elements: state (k, b) carries the weight A_g(k, b) = sum_{i in group g} |U[k][i][b]|^2
 * (U: the eigenvectors of tbk_eigh, convention 2), and A_g is interpolated linearly inside the simplices of tbk_dos like the band
 * energy (Bloechl's corner weights; csrc/tbk_pdos.hip).  mesh, the energy grid and the simplices are those of
 * tbk_dos.
 *   groups  n_groups in [1, TBK_PDOS_MAX_GROUPS]; group g = group_orbitals[group_offsets[g] .. group_offsets[g + 1]): int32 indices
 *           in [0, n_orb), at least one per group, none twice inside a group (group_offsets[0] == 0; an orbital may sit in several
 *           groups or in none)
 *   nos     double [n_groups][n_e]  nos[g][j] = states per unit cell with energy <= E_j weighted by A_g; over groups that partition
 *           the orbitals the rows add up to the nos of tbk_dos
 * Inside a degenerate eigenspace the split of A_g over the bands depends on the basis tbk_eigh returns; its sum over the cluster
 * does not, and nos moves by no more than the method's own discretisation error.
 * The kernels accumulate in 64-bit fixed point (2^-40 per contribution, |error| <= 9.1e-13 n_orb) and sum in integers: for given
 * (E, W) the same call gives the same bits.  Energy grids are tiled by 4096 / GT points per workgroup, GT = n_groups rounded up to
 * a power of two.
 * Argument errors (TBK_ERR_ARGUMENT): those of tbk_dos, n_groups outside [1, TBK_PDOS_MAX_GROUPS], an empty group, an index outside
 * [0, n_orb), a repeat inside a group, a NULL pointer, a k.p handle, more than 2^42 (simplex, band) pairs.  Host buffers;
 * synchronous. */
enum { TBK_PDOS_MAX_GROUPS = 16 };

/* The accumulate stage alone on an eigensystem the caller brings: E[NK][n_orb] in mesh order, every row ascending, and the weights
 * W[NK][n_groups][n_orb] in [0, 1] (what tbk_dos_from_eigenvalues is to tbk_dos: for tests, and for callers with their own
 * weights -- spin, layer or any other diagonal observable). */
int tbk_pdos_from_eigensystem(int device, int dim, const int32_t* mesh, int n_orb, int n_groups, const double* E, const double* W,
                              double e_min, double e_step, int64_t n_e, double* nos_out);
/* The whole call: the mesh's k list is made on the host and walked in chunks of at most TBK_OPT_K_CHUNK k-points (0: chosen from
 * free device memory; chunks need not be whole mesh planes); per chunk tbk_eigh_device fills a chunk-sized eigenvector workspace
 * and one kernel reduces it to the chunk's rows of W.  E and W of the whole mesh stay in device memory (NK n_orb (1 + n_groups)
 * doubles; TBK_ERR_MEMORY when they, or the eigenvectors of one chunk, do not fit); all eigenvectors are never held.  Non-finite
 * eigenvalues and no convergence are reported as by tbk_eigh, in front of the accumulate kernels.  The eigenvector solver is the one
 * tbk_eigh takes (Jacobi up to 64 orbitals, whose result for a matrix does not depend on the chunk; rocSOLVER above). */
int tbk_pdos(tbk_model* m, const int32_t* mesh, const int32_t* group_offsets, const int32_t* group_orbitals, int n_groups,
             double e_min, double e_step, int64_t n_e, double* nos_out);
/* On several devices from one process: the slabs of tbk_dos_multi (handle i: ceil(n_1 / n_handles) cells along axis 0 plus the
 * periodic neighbour plane), the host adds the handles' shares in handle order, empty slabs are skipped.  n_handles == 1 is
 * tbk_pdos. */
int tbk_pdos_multi(tbk_model* const* handles, int n_handles, const int32_t* mesh, const int32_t* group_offsets,
                   const int32_t* group_orbitals, int n_groups, double e_min, double e_step, int64_t n_e, double* nos_out);
/* While TBK_OPT_TIMING is on: ms[3] = summed HIP-event time of this handle's tbk_pdos calls in the weights kernel (all chunks), the
 * accumulate kernel, and the reduction + prefix sum; calls = how many; reset = 1 clears.  (The eigenvector stages are in
 * tbk_get_timing.) */
int tbk_pdos_timing(tbk_model* m, double* ms, int64_t* calls, int reset);

/* ---- band edges and the Fermi level of a uniform k mesh (not in the reference) ---------------------------------------------------
 * mesh, the simplices and the filled fraction n_T(E) of a simplex are those of tbk_dos; N(E) = 1 / (S NK) sum n_T(E) counts states
 * without a spin factor (csrc/tbk_fermi.hip).  There is no energy grid: the kernel evaluates N at up to 16
 * arbitrary energies per launch, in registers, and produces per energy the integer
 *     Q(E) = sum over (cell, band, simplex) of round(n_T(E) 2^40) [e1 <= E < e_top]  +  2^40 * (simplices with e_top <= E),
 * independent of wave order, of the workgroup count and of the other energies of the launch; N(E) = Q(E) / (2^40 S NK), rounded
 * twice (|N - exact| <= 4.5e-13 n_orb from the fixed point).
 *   band edges   emin[b] = min over the mesh points of E[k][b], emax[b] = max: doubles of the eigenvalue array, no arithmetic
 *   Fermi level  for n_electrons = n in (0, n_orb), target t = n S NK 2^40:
 *     gap case   n is an integer m and emax[m - 1] < emin[m]: lower = emax[m - 1], upper = emin[m], mu = lower + (upper - lower) / 2,
 *                N(mu) = m; no kernel pass.  (Fixed point cannot find a band edge: 1 - (y / gap)^3 rounds to 1 at 2^-40 once
 *                y / gap < 1e-4.)
 *     otherwise  mu = lower = upper = the double hi of a bracket lo < hi of NEIGHBOURING doubles with Q(lo) < t <= Q(hi), found
 *                from lo = nextafter(emin[0], -inf), hi = emax[n_orb - 1] in passes of 15 probes that are equidistant in the
 *                ordered-integer image of the doubles (a bracket around zero first takes one pass at 0 and lo, hi times 2^-256 j,
 *                j = 1 .. 7): at most 16 passes whatever the scale, and a scaling of all energies by a power of two moves the
 *                probes with it.  N(mu) is the kernel's value at hi.
 *     Q against t  exactly, in integers: Q is kept as (whole, rem) with Q = whole 2^40 + rem, rem < 2^40 -- whole = count + the
 *                fraction words' carry -- and t is replaced by the integer ceil(t) in the same form (Q is an integer, so
 *                Q >= t <=> Q >= ceil(t)); Q >= t <=> whole > t.whole or (whole == t.whole and rem >= t.rem).  S NK n_orb 2^40 does
 *                not fit 64 bits; no product of the two words is formed.  Several handles: the pairs are added, with carry.
 *     flat band  across a band that is constant over the mesh N jumps; for n inside the jump mu is the energy of the jump and
 *                N(mu) the value above it.  Not an error.
 * Range: as for tbk_dos, eigenvalues and probe energies must stay below 2^969 in magnitude (not checked).
 * Argument errors (TBK_ERR_ARGUMENT): dim not in {2, 3}, a mesh entry < 1, 2^31 mesh points or more, n_electrons not finite or
 * outside (0, n_orb), a probe energy that is not finite, n_p < 1, a NULL pointer, a k.p handle, a handle given twice.  Host buffers;
 * synchronous. */

/* The probe kernel alone on eigenvalues the caller brings (E[NK][n_orb] in mesh order, every row ascending): nos_out[j] = N(energies[j])
 * for n_p >= 1 finite energies in any order, walked 16 per launch.  The value at an energy does not depend on the others. */
int tbk_nos_at_from_eigenvalues(int device, int dim, const int32_t* mesh, int n_orb, const double* E, const double* energies,
                                int64_t n_p, double* nos_out);
/* emin_out / emax_out: double [n_orb] */
int tbk_band_edges_from_eigenvalues(int device, int dim, const int32_t* mesh, int n_orb, const double* E, double* emin_out,
                                    double* emax_out);
/* out: double [4] = mu, lower, upper, N(mu); passes_out (may be NULL): the kernel passes of the search, 0 in the gap case */
int tbk_fermi_from_eigenvalues(int device, int dim, const int32_t* mesh, int n_orb, const double* E, double n_electrons, double* out,
                               int32_t* passes_out);
/* The whole call: the mesh is evaluated as in tbk_dos (fold hint, tbk_eigenval_check in front of the kernels), and its eigenvalues
 * stay in device memory across all passes. */
int tbk_band_edges(tbk_model* m, const int32_t* mesh, double* emin_out, double* emax_out);
int tbk_fermi(tbk_model* m, const int32_t* mesh, double n_electrons, double* out);
/* On several devices from one process: the slabs of tbk_dos_multi.  Every handle keeps its slab's eigenvalues and probes them in
 * every pass (its periodic neighbour plane is read by its last cells and left out of its band edges); the host adds the handles'
 * integer pairs and takes the min / max of their edges, so for given eigenvalues the handle count changes no bit -- the
 * eigenvalues themselves differ at rounding level between handle counts, as for tbk_dos_multi.  The calling thread holds every
 * handle for the whole call and drives them all: the handles must be distinct. */
int tbk_band_edges_multi(tbk_model* const* handles, int n_handles, const int32_t* mesh, double* emin_out, double* emax_out);
int tbk_fermi_multi(tbk_model* const* handles, int n_handles, const int32_t* mesh, double n_electrons, double* out);
/* calls = this handle's tbk_fermi / tbk_band_edges calls, passes = the kernel passes of its searches, ms = the summed HIP-event time
 * of its probe and band-edge kernels in the calls made while TBK_OPT_TIMING was on; reset = 1 clears. */
int tbk_fermi_timing(tbk_model* m, double* ms, int64_t* calls, int64_t* passes, int reset);

/* ---- tetrahedron integration weights and occupations of a uniform k mesh (not in the reference) -----------------------------------
 * mesh, the simplices, the half-open ranges and the stable sort are those of tbk_dos / tbk_pdos (csrc/tbk_occ.hip, DESIGN.md
 * section 13).  At one energy mu every state (k, b) of the mesh gets the weight
 *     w[k][b] = 1 / (S NK) * sum over the simplices T that contain mesh point k of Bloechl's corner weight of k in T,
 * 24 tetrahedra over 15 mesh points in three dimensions, 6 triangles over 7 in two, added in one fixed order and divided once:
 * sum_{k, b} w = N(mu), 0 <= NK w <= 1, w = 0 exactly below the spectrum and the double nearest 1 / NK above it.  Any
 * Brillouin-zone integral over the occupied states is then sum_{k, b} w[k][b] A[k][b]; three of them are computed here:
 *     f[b]  = sum_k w[k][b]                          band occupations in [0, 1] (fixed point 2^-40: exactly 1 for a full band)
 *     eb[b] = sum_k w[k][b] E[k][b]                  band energies (doubles, in an order fixed by the mesh and n_orb)
 *     q[i]  = sum_k sum_b w[k][b] |U[k][i][b]|^2     orbital occupations, U of tbk_eigh, convention 2 (fixed point: for given
 *                                                    (w, U) the same bits for every chunk size; |error| <= 2^-41 per orbital)
 * sum_i q[i] = sum_b f[b] = N(mu).  Inside a degenerate eigenspace the split of q over the bands depends on the basis the
 * eigensolver returns (the caveat of tbk_pdos); the sum over the degenerate cluster does not.
 * Argument errors (TBK_ERR_ARGUMENT), before any device is touched: dim not in {2, 3}, a mesh entry < 1, 2^31 mesh points or more,
 * an energy that is not finite, mode not in {0, 1}, mode 1 with n_electrons not finite or outside (0, n_orb), k_chunk < 0, a NULL
 * pointer, a k.p handle, a handle given twice.  Host buffers; synchronous. */

/* The kernels alone on an eigensystem the caller brings: E[NK][n_orb] in mesh order, rows ascending; U[NK][n_orb][n_orb][2] with
 * U[k][i][b] = component i of band b.  w_out: double [NK][n_orb].  U is walked in chunks of k_chunk mesh points (0: all at once);
 * q_out, f_out, eb_out: double [n_orb]. */
int tbk_tetra_weights_from_eigenvalues(int device, int dim, const int32_t* mesh, int n_orb, const double* E, double energy, double* w_out);
int tbk_occupations_from_eigensystem(int device, int dim, const int32_t* mesh, int n_orb, const double* E, const double* U, double energy,
                                     int64_t k_chunk, double* q_out, double* f_out, double* eb_out);
/* The whole call: the mesh is evaluated through the eigenvalue path as in tbk_fermi (fold hint, tbk_eigenval_check in front of the
 * kernels), so tbk_tetra_weights, tbk_fermi and tbk_occupations see the same eigenvalues.  tbk_tetra_weights is the one call of the
 * family that returns NK n_orb doubles.  tbk_occupations: mode 0, value = the energy mu, mu_out = (mu, mu, mu, N(mu)) with N from the
 * probe kernel of tbk_fermi; mode 1, value = n_electrons, mu_out = the four numbers of tbk_fermi, whose search runs on the resident
 * eigenvalues.  The weights stay in device memory; the k list is walked in chunks of at most TBK_OPT_K_CHUNK points (0: what
 * tbk_eigh_device would choose), per chunk tbk_eigh_device fills a chunk-sized eigenvector workspace that one kernel contracts
 * with the chunk's weights.  Memory: 2 NK n_orb doubles and the eigenvectors of one chunk (TBK_ERR_MEMORY otherwise). */
int tbk_tetra_weights(tbk_model* m, const int32_t* mesh, double energy, double* w_out);
int tbk_occupations(tbk_model* m, const int32_t* mesh, int mode, double value, double* mu_out, double* q_out, double* f_out,
                    double* eb_out);
/* On several devices from one process: the slabs of tbk_dos_multi.  A handle keeps its slab's eigenvalues and the periodic
 * neighbour plane on BOTH sides, and writes weights for its own planes only; the host concatenates w, adds the integer words of f
 * and q exactly and adds eb in handle order.  The calling thread holds every handle for the whole call: the handles must be
 * distinct. */
int tbk_tetra_weights_multi(tbk_model* const* handles, int n_handles, const int32_t* mesh, double energy, double* w_out);
int tbk_occupations_multi(tbk_model* const* handles, int n_handles, const int32_t* mesh, int mode, double value, double* mu_out,
                          double* q_out, double* f_out, double* eb_out);
/* ms[3] = the summed HIP-event time of the weights kernel, the band sums, and the contraction + its reduction in this handle's calls
 * made while TBK_OPT_TIMING was on; calls = how many calls; reset = 1 clears.  (The eigensolver stages are in tbk_get_timing.) */
int tbk_occ_timing(tbk_model* m, double* ms, int64_t* calls, int reset);

/* ---- the real-space density matrix of a uniform k mesh (not in the reference) --------------------------------------------------
 * Mesh, simplices, the weights w[k][b] at mu and the eigenvectors U[k][i][b] (convention 2) are those of tbk_occupations
 * (csrc/tbk_dm.hip).  With the mesh points k = (i_1 / n_1, ..., i_dim / n_dim):
 *     P(k)[i][j]   = sum_b w[k][b] U[k][i][b] conj(U[k][j][b])                         Hermitian, trace = sum_b w[k][b]
 *     rho(R)[i][j] = sum_k exp(-2 pi i sum_d ((i_d R_d) mod n_d) / n_d) P(k)[i][j]     for every requested integer vector R
 * The argument of the phase is reduced in integers: every (i_d R_d) mod n_d is taken in 64-bit arithmetic with a non-negative
 * result, the numerators are brought to the common denominator NK = prod n_d and reduced modulo NK, and cos / sin are taken of
 * that fraction; rho(R + n_d e_d) has the bits of rho(R).  rho(-R) = rho(R)^H, diag rho(0) = the q of tbk_occupations, tr rho(0) =
 * N(mu); with the stored half of the hoppings sum_b eb[b] = 2 Re sum_R sum_ij conj(rho(R)[i][j]) hop[R][i][j].  Every element is
 * a sum of NK n_orb terms whose moduli add up to at most 1: |error| <= 4 (NK n_orb + 32) 2^-53.  Repeated calls with the same
 * arguments, chunk size and handles give the same bits; another chunk size regroups the sums (inside the bound).  The split of a
 * degenerate cluster's weight over its bands depends on the basis the eigensolver returns (the caveat of tbk_occupations); rho of a
 * cluster filled as a whole does not.
 * R: int64 [n_r][dim], duplicates allowed; rho_out: double [n_r][n_orb][n_orb][2].  Argument errors (TBK_ERR_ARGUMENT), before any
 * device is touched: those of tbk_occupations, n_r < 1 or above 1048560, more than 16320 orbitals, a NULL pointer.  rho, its partial
 * sums (at most 256 MiB beyond rho itself) and the buffers of one k chunk must fit (TBK_ERR_MEMORY otherwise).  Host buffers;
 * synchronous. */

/* The kernels alone on an eigensystem the caller brings (E, U, k_chunk as for tbk_occupations_from_eigensystem). */
int tbk_density_matrix_from_eigensystem(int device, int dim, const int32_t* mesh, int n_orb, const double* E, const double* U, double energy,
                                        int64_t k_chunk, int64_t n_r, const int64_t* R, double* rho_out);
/* The whole call: eigenvalues, mu (mode, value, mu_out as for tbk_occupations: mode 1 gives tbk_fermi's numbers bit for bit) and the
 * weights as in tbk_occupations; then the k list is walked in chunks of at most TBK_OPT_K_CHUNK points (0: half of what
 * tbk_eigh_device would choose, the projectors of a chunk take the other half), per chunk tbk_eigh_device, the chunk's phase table,
 * its projectors and their contraction into the resident rho. */
int tbk_density_matrix(tbk_model* m, const int32_t* mesh, int mode, double value, int64_t n_r, const int64_t* R, double* mu_out,
                       double* rho_out);
/* On several devices from one process: the slabs of tbk_dos_multi.  Every handle contracts the mesh points of its own planes, the host
 * adds the handles' partial rho in handle order.  The handles must be distinct. */
int tbk_density_matrix_multi(tbk_model* const* handles, int n_handles, const int32_t* mesh, int mode, double value, int64_t n_r,
                             const int64_t* R, double* mu_out, double* rho_out);
/* How the contraction over k of a slab of `rows` mesh points is cut: out[0] = n_r rounded up to the tile of 16, out[1] = the k slices
 * (one partial rho each, added in index order; 1: none), out[2] = mesh points per slice.  A function of its arguments alone. */
int tbk_dm_plan(int64_t rows, int n_orb, int64_t n_r, int64_t* out);
/* ms[3] = the summed HIP-event time of the phase tables, the projectors, and the contraction + the sum of its slices in this handle's
 * calls made while TBK_OPT_TIMING was on; calls = how many calls; reset = 1 clears.  (The eigensolver stages are in tbk_get_timing; the
 * weights kernel, a stage of tbk_occ_timing, is not timed in these calls.) */
int tbk_dm_timing(tbk_model* m, double* ms, int64_t* calls, int reset);

/* ---- the lattice Green's function (the resolvent) of a uniform k mesh at complex energies (not in the reference) -----------------
 * Mesh and mesh points k = (i_1 / n_1, ..., i_dim / n_dim) are those of tbk_occupations (dim 2 or 3), E and U those of
 * tbk_eigh_device with convention 2, the phase is the integer-reduced one of tbk_density_matrix (R + n_d e_d gives the bits of R):
 *
 *     G(R, z)[i][j] = sum_k exp(-2 pi i k . R) sum_b (1 / (z - E[k][b]) / NK) U[k][i][b] conj(U[k][j][b])
 *
 * z: double [n_z][2] (re, im), 1 <= n_z <= 4096, every component finite and every Im z != 0 (either sign), else TBK_ERR_ARGUMENT
 * before any device is touched.  R: int64 [n_r][dim], n_r as for tbk_density_matrix.  G_out: double [n_r][n_z][n_orb][n_orb][2].
 * Per chunk of k-points the phase table is made once; per tile of at most 4 energies one projector launch (the eigenvectors of a
 * block go through LDS once per tile) and one Fourier contraction into partial sums that stay resident across the chunks.  For a
 * given eigensystem, chunk size and slab the bits of G(R, z) depend on (R, z) alone: not on the other energies, their order or
 * the tile.  Error for a given eigensystem: 4 (NK n_orb + 32) 2^-53 / min |Im z| per component. */

/* The kernels alone on an eigensystem the caller brings (E [NK][n_orb], U [NK][n_orb][n_orb][2]).  k_chunk, z_tile: 0 means
 * tbk_green_plan's; a z_tile above 4 is 4. */
int tbk_green_from_eigensystem(int device, int dim, const int32_t* mesh, int n_orb, const double* E, const double* U, int64_t k_chunk,
                               int64_t z_tile, int64_t n_z, const double* z, int64_t n_r, const int64_t* R, double* G_out);
/* The whole call: the partial sums and G are reserved and cleared, then the k list is walked in chunks of at most TBK_OPT_K_CHUNK
 * points (0: chosen from the memory left, shared between the chunk's eigenvectors and the projectors of one tile), per chunk
 * tbk_eigh_device, the phase table and, per energy tile, projectors and contraction.  TBK_ERR_MEMORY when G, its partials (about
 * slices x n_r x n_z x n_orb^2 complex numbers) or one chunk do not fit. */
int tbk_green_function(tbk_model* m, const int32_t* mesh, int64_t n_z, const double* z, int64_t n_r, const int64_t* R, double* G_out);
/* On several devices from one process: the slabs of tbk_dos_multi, added by the host in handle order.  The handles must be distinct. */
int tbk_green_function_multi(tbk_model* const* handles, int n_handles, const int32_t* mesh, int64_t n_z, const double* z, int64_t n_r,
                             const int64_t* R, double* G_out);
/* How a slab of `rows` mesh points is worked: out[0 .. 2] = tbk_dm_plan(rows, n_orb, n_r) (the k slices do not depend on the
 * energies), out[3] = energies per tile (z_tile, 0: 4; at most n_z, and at most what keeps the projectors of one chunk of k_chunk
 * points inside 1 GiB), out[4] = tiles, out[5] = k-points per chunk (k_chunk, 0: rows, capped so that the projectors of one tile
 * stay inside 1 GiB; never more than the phase table's budget allows), out[6] = the projector template: 1 (n_orb <= 16: 16 x 16
 * blocks of four k-points) or 4 (64 x 64 blocks).  A function of its arguments alone. */
int tbk_green_plan(int64_t rows, int n_orb, int64_t n_r, int64_t n_z, int64_t z_tile, int64_t k_chunk, int64_t* out);
/* ms[3] = the summed HIP-event time of the phase tables, the projectors, and the contractions + the sums of their slices in this
 * handle's calls made while TBK_OPT_TIMING was on; calls = how many calls; reset = 1 clears.  (The eigensolver stages are in
 * tbk_get_timing.) */
int tbk_green_timing(tbk_model* m, double* ms, int64_t* calls, int reset);

/* ---- the dressed lattice Green's function: a local, energy-dependent self-energy by batched inversion (not in the reference) ------
 * Mesh, mesh points, phase, R, G_out and the energy tiles are those of tbk_green_function; H(k) is that of tbk_hamilton_device with
 * convention 2; Sigma: double [n_z][n_orb][n_orb][2], any finite complex matrices (not Hermitian, not causal if the caller says so):
 *
 *     G(R, z) = sum_k exp(-2 pi i k . R) (z 1 - H(k) - Sigma(z))^-1 / NK
 *
 * z: double [n_z][2], 1 <= n_z <= 4096, every component finite; Im z = 0 is allowed here (Sigma carries its own broadening).  No
 * eigensolve: per chunk the FULL H(k), per energy tile one launch of the inversion kernel (Gauss-Jordan in place, partial pivoting on
 * |re| + |im| with ties to the lowest row, panels of 16 pivots whose rank-16 update runs on the FP64 matrix pipe; up to 64 orbitals)
 * and one Fourier contraction.  Above 64 orbitals, and for a handle with TBK_OPT_EIGENSOLVER = TBK_EIG_ROCSOLVER,
 * rocsolver_zgetrf / zgetri_strided_batched take the inversions (booked on TBK_CNT_LIBRARY_CALLS).  A pivot that is exactly zero, a
 * library status != 0 or a non-finite element of an inverse is TBK_ERR_SINGULAR; the message names the first such mesh point and
 * energy, and G_out is not to be used.  The bits of G(R, z) depend on (R, z, Sigma(z)) alone for a given H, chunk size and slab.
 * Error per component: max_k 8 n u rho kappa_2(A) ||A^-1||_2 + 4 (NK + 32) u max_k ||A^-1||_2. */

/* The kernels alone on matrices the caller brings (H [NK][n_orb][n_orb][2] in mesh order).  k_chunk, z_tile: as for
 * tbk_green_from_eigensystem.  Always the own kernel up to 64 orbitals, the library above. */
int tbk_green_dressed_from_matrices(int device, int dim, const int32_t* mesh, int n_orb, const double* H, int64_t k_chunk, int64_t z_tile,
                                    int64_t n_z, const double* z, const double* Sigma, int64_t n_r, const int64_t* R, double* G_out);
/* The whole call: the loop of tbk_green_function with H(k) of the chunk and the inversions in the place of the eigensolve and the
 * projectors.  The chunk (TBK_OPT_K_CHUNK, 0: from the memory left) is shared between H(k) of the chunk and the inverses of one tile. */
int tbk_green_dressed(tbk_model* m, const int32_t* mesh, int64_t n_z, const double* z, const double* Sigma, int64_t n_r, const int64_t* R,
                      double* G_out);
/* On several devices from one process: the slabs of tbk_dos_multi, added by the host in handle order.  The handles must be distinct. */
int tbk_green_dressed_multi(tbk_model* const* handles, int n_handles, const int32_t* mesh, int64_t n_z, const double* z, const double* Sigma,
                            int64_t n_r, const int64_t* R, double* G_out);
/* ms[3] = the summed HIP-event time of the phase tables, the inversions (with the library route: forming, LU, inverse and scatter), and
 * the contractions + the sums of their slices in this handle's dressed calls made while TBK_OPT_TIMING was on; calls, reset as above.
 * (H(k) is in tbk_get_timing.) */
int tbk_green_dressed_timing(tbk_model* m, double* ms, int64_t* calls, int reset);

/* ---- surface and bulk Green's functions of a semi-infinite crystal by iterative decimation (not in the reference) -------------------
 * Lopez Sancho, Lopez Sancho and Rubio, J. Phys. F 15, 851 (1985).  With a the stacking axis, hop_full[R] the full hopping matrices
 * (tbk_hamilton with convention 2 is sum_R exp(2 pi i k.R) hop_full[R]) and kp an in-plane point (the reduced coordinates without
 * component a):
 *
 *     H_m(kp)   = sum_{R : R_a = m} exp(2 pi i kp.Rp) hop_full[R]        m = -L ... L;  L = layers >= max |R_a|
 *     H00[p][q] = H_{q-p},  H01[p][q] = H_{L+q-p} for q <= p, else 0     blocks of n_orb x n_orb, p, q = 0 ... L - 1;  N = n_orb max(L, 1)
 *
 *     es = et = e = H00, alpha = H01, beta = H01^H;  repeat  g = (z 1 - e)^-1,  T = g alpha:  alpha' = alpha T, et += beta T, e += beta T,
 *     T = g beta:  es += alpha T, e += alpha T, beta' = beta T  until, after an update, max(|alpha|_inf, |beta|_inf) <= 2^-53 |H01|_inf
 *     (row sums of |re| + |im|);   bottom = (z - es)^-1,  top = (z - et)^-1,  bulk = (z - e)^-1.
 *
 * bottom: the crystal on principal layers P >= 0 (its surface cell is block 0); top: on P <= 0 (surface cell: block L - 1); bulk: a
 * principal layer deep inside.  L = 0: no iteration, all three are (z - H00)^-1.  z: double [n_z][2], 1 <= n_z <= 4096, finite,
 * Im z != 0.  max_iterations: 1 ... 4096; a (kp, z) that reaches it is TBK_ERR_NO_CONVERGENCE, a zero pivot or a non-finite element of
 * an inverse TBK_ERR_SINGULAR; the message names the first such k index and energy, and the results are not to be used.  Results:
 * iterations int32 [nk][n_z]; bottom, top, bulk double [nk][n_z][N][N][2] or, spectral != 0, double [nk][n_z][N] holding -Im diag / pi
 * (no matrix leaves the device).  The bits of one (kp, z) depend on nothing else.  N <= 64: one workgroup per (kp, z), Gauss-Jordan
 * of tbk_green_dressed, six products per iteration on the FP64 matrix pipe.  65 <= N <= 1024, and for a handle with
 * TBK_OPT_EIGENSOLVER = TBK_EIG_ROCSOLVER: the (kp, z) of a chunk in lockstep, in batches of a fixed number of members, on
 * rocblas_zgemm_strided_batched and rocsolver_zgetrf / zgetri_strided_batched (booked on TBK_CNT_LIBRARY_CALLS); a member that has
 * converged gets alpha = beta = 0 exactly.  N > 1024 is TBK_ERR_ARGUMENT.
 * Error per component: 8 N u rho (|z| + |H00|_2 + 2 |H01|_2) / (Im z)^2 (iterations + 1). */

/* The kernel alone on principal layers the caller brings: H00, H01 double [n_k][N][N][2] (H01 NULL: no hopping between the layers, no
 * iteration).  k_chunk: points per launch (0: from the size of the results).  Always the own kernel up to 64 rows, the library above. */
int tbk_surface_from_matrices(int device, int N, int64_t n_k, const double* H00, const double* H01, int64_t n_z, const double* z,
                              int max_iterations, int64_t k_chunk, int spectral, int32_t* iterations, double* bottom, double* top, double* bulk);
/* The whole call: k double [nk][dim - 1] (dim = 1: ignored, nk = 1 is the one point there is).  Per chunk (TBK_OPT_K_CHUNK, 0: from the
 * size of the results) the FULL H(k) of tbk_hamilton_device at k_a = j / (2 layers + 1), j = 0 ... 2 layers, H_m from them by a discrete
 * Fourier sum, then the decimation.  layers below the reach of a stored hopping vector along axis is TBK_ERR_ARGUMENT. */
int tbk_surface_green(tbk_model* m, int axis, int layers, const double* k, int64_t nk, int64_t n_z, const double* z, int max_iterations,
                      int spectral, int32_t* iterations, double* bottom, double* top, double* bulk);
/* On several devices from one process: the slabs of tbk_hamilton_multi, every device writing its rows of the results. */
int tbk_surface_green_multi(tbk_model* const* handles, int n_handles, int axis, int layers, const double* k, int64_t nk, int64_t n_z,
                            const double* z, int max_iterations, int spectral, int32_t* iterations, double* bottom, double* top, double* bulk);
/* ms[3] = the summed HIP-event time of H(k) with the principal layers, the decimation, and the copies of the results to the host in this
 * handle's calls made while TBK_OPT_TIMING was on; calls, reset as above. */
int tbk_surface_timing(tbk_model* m, double* ms, int64_t* calls, int reset);

/* ---- Landauer transmission through a device of M principal layers between two semi-infinite leads (not in the reference) ------------
 * H00, H01, N, L and the decimation with its stopping rule are those of tbk_surface_green (layers >= 1: there must be hopping along the
 * axis).  The device is the principal layers p = 1 ... M with on-site blocks H00(kp) + V_p, V_p a Hermitian N x N matrix independent
 * of kp and ordered in blocks as H00; H01 between neighbouring layers and towards both leads; the left lead is the crystal on the
 * layers P <= 0, the right lead on P >= M + 1.  Per (kp, z), Im z != 0:
 *
 *     es, et, iterations from the decimation (without its closing inversions);  Gamma_R = i (es - es^H),  Gamma_L = i (et - et^H)
 *     D_1 = et + V_1;  for p = 1 ... M:  (p = M: D_p += es - H00)   g_p = (z - D_p)^-1
 *                                        P_p = g_p (p = 1),  g_p (H01^H P_{p-1}) (p > 1);   D_{p+1} = (H00 + V_{p+1}) + H01^H (g_p H01)
 *     T = Re tr[(Gamma_R P_M) (Gamma_L P_M^H)]
 *
 * P_M is block (M, 1) of the resolvent of the device with both lead self-energies attached.  V: double [M][N][N][2], 1 <= M <= 4096 and
 * at most 256 MiB, staged once per call.  Results: iterations int32 [nk][n_z], T double [nk][n_z] and, G not NULL, P_M as double
 * [nk][n_z][N][N][2]; without G one double per (kp, z) leaves the device.  The cap of the decimation is TBK_ERR_NO_CONVERGENCE; a zero
 * pivot or a non-finite element of any g_p or of P_M is TBK_ERR_SINGULAR; the message names the first such k index and energy.  The bits
 * of one (kp, z) depend on nothing else.  N <= 64: one workgroup owns a (kp, z) from the first decimation step to the trace.  65 <= N <=
 * 1024, and for a handle with TBK_OPT_EIGENSOLVER = TBK_EIG_ROCSOLVER: the lead part of tbk_surface_green's library route, then M
 * lockstep rounds of zgetrf / zgetri and four zgemm_strided_batched (booked on TBK_CNT_LIBRARY_CALLS).  H01 NULL, layers = 0, M outside
 * [1, 4096], V above 256 MiB and N > 1024 are TBK_ERR_ARGUMENT.
 * Error: |T - exact| <= 4 eps scale, eps = 8 N u rho (|z| + |H00|_2 + 2 |H01|_2 + max |V_p|_2) / |Im z| (iterations + M + 1), scale =
 * N (2 |H01|^2 |G_bottom|) (2 |H01|^2 |G_top|) |P_M|^2. */

/* The kernel alone on principal layers the caller brings: H00, H01 double [n_k][N][N][2].  k_chunk: points per launch (0: from the size
 * of the results).  Always the own kernel up to 64 rows, the library above. */
int tbk_transmission_from_matrices(int device, int N, int64_t n_k, const double* H00, const double* H01, int M, const double* V, int64_t n_z,
                                   const double* z, int max_iterations, int64_t k_chunk, int32_t* iterations, double* T, double* G);
/* The whole call: k, layers, the chunks and H_m as in tbk_surface_green. */
int tbk_transmission(tbk_model* m, int axis, int layers, const double* k, int64_t nk, int M, const double* V, int64_t n_z, const double* z,
                     int max_iterations, int32_t* iterations, double* T, double* G);
/* On several devices from one process: the slabs of tbk_hamilton_multi, every device writing its rows of the results. */
int tbk_transmission_multi(tbk_model* const* handles, int n_handles, int axis, int layers, const double* k, int64_t nk, int M, const double* V,
                           int64_t n_z, const double* z, int max_iterations, int32_t* iterations, double* T, double* G);
/* ms[3] = the summed HIP-event time of H(k) with the principal layers, the decimation with the sweep (one launch on the own kernel's
 * route, so the two are not separated), and the copies of the results to the host in this handle's calls made while TBK_OPT_TIMING was
 * on; calls, reset as above. */
int tbk_transmission_timing(tbk_model* m, double* ms, int64_t* calls, int reset);

/* ---- the transmission of an ensemble of devices: disorder samples after one decimation (not in the reference) ------------------------
 * T[k][z][s], s = 0 ... n_s - 1, is tbk_transmission's T of the device V_s, unchanged down to the order of the operations: up to
 * N = 64 every T[k][z][s] and iterations[k][z] have the bits of tbk_transmission called with V_s alone.  The decimation of a (kp, z)
 * does not depend on V: it is computed once for a group of samples, and the sweep with its closing once per sample.  Exactly one of
 *     V       double [n_s][M][N][N][2]   Hermitian matrices, as tbk_transmission's
 *     onsite  double [n_s][M][N]         real on-site energies: they stay diagonal into the kernel, which adds the energy on the
 *                                        diagonal and 0.0 elsewhere in the expressions of the matrix form -- the bits are those of
 *                                        the matrix form on the expanded diagonal
 * is not NULL.  Results: iterations int32 [nk][n_z], T double [nk][n_z][n_s]; n_s doubles per (kp, z) leave the device.  A work item
 * of the own kernel (N <= 64) is (kp, z, a group of consecutive samples); the group that holds sample 0 writes iterations.  The bits
 * of a T[k][z][s] depend on nothing else: not on the groups, the chunks, the grid, the other samples or their order.  Above N = 64,
 * and for a handle with TBK_OPT_EIGENSOLVER = TBK_EIG_ROCSOLVER, the library route of tbk_transmission runs its decimation once per
 * lockstep batch and its sweep once per sample; there are no groups there.
 * Errors: tbk_transmission's, and TBK_ERR_ARGUMENT for both or none of V and onsite, n_s outside [1, 4096], sample_chunk < 0 and more
 * than 256 MiB of staged devices.  The message of TBK_ERR_SINGULAR names the k index, the energy and the sample (the smallest such
 * triple in that order; a singular decimation names sample 0), that of TBK_ERR_NO_CONVERGENCE the k index and the energy.  Error
 * bound per sample: tbk_transmission's. */

/* The kernel alone on principal layers the caller brings: H00, H01 double [n_k][N][N][2], n_k < 2^36.  k_chunk: points per launch
 * (0: from the size of the results, n_z (8 n_s + 4) bytes per point).  sample_chunk: samples per workgroup visit (0: chosen so that
 * the groups of a chunk fill the workgroups resident at once and no further: every extra group repeats the decimation). */
int tbk_transmission_ensemble_from_matrices(int device, int N, int64_t n_k, const double* H00, const double* H01, int M, int64_t n_s, const double* V,
                                            const double* onsite, int64_t n_z, const double* z, int max_iterations, int64_t k_chunk,
                                            int64_t sample_chunk, int32_t* iterations, double* T);
/* The whole call: k, layers, the chunks and H_m as in tbk_surface_green; the groups are chosen as for sample_chunk = 0. */
int tbk_transmission_ensemble(tbk_model* m, int axis, int layers, const double* k, int64_t nk, int M, int64_t n_s, const double* V, const double* onsite,
                              int64_t n_z, const double* z, int max_iterations, int32_t* iterations, double* T);
/* On several devices from one process: the slabs of tbk_hamilton_multi; every handle stages all the samples. */
int tbk_transmission_ensemble_multi(tbk_model* const* handles, int n_handles, int axis, int layers, const double* k, int64_t nk, int M, int64_t n_s,
                                    const double* V, const double* onsite, int64_t n_z, const double* z, int max_iterations, int32_t* iterations,
                                    double* T);
/* ms[3] = the summed HIP-event time of H(k) with the principal layers, the decimation with the sweeps of every sample, and the copies
 * of the results to the host in this handle's calls made while TBK_OPT_TIMING was on; calls, reset as above.  A row of its own:
 * tbk_transmission_timing does not count these calls. */
int tbk_transmission_ensemble_timing(tbk_model* m, double* ms, int64_t* calls, int reset);

/* ---- the transmission eigenvalues of an ensemble of devices: channels and shot noise (not in the reference) ---------------------------
 * channels[k][z][s][0 ... N) are the transmission eigenvalues T_n of the device V_s in descending order: the eigenvalues of t^H t,
 * t = L_R^H (P_M L_L), whose trace is tbk_transmission's T.  Per (kp, z, sample), behind the decimation and the sweep of
 * tbk_transmission_ensemble, unchanged and in their order, with s = sign(Im z):
 *
 *     B_R = s i (es - es^H),  B_L = s i (et - et^H)     Hermitian, positive semidefinite up to rounding for either sign of Im z
 *     B = L L^H        Cholesky with diagonal pivoting: the largest remaining diagonal first (ties: the lowest index, a NaN counts as
 *                      +inf); it stops at rank r when that diagonal is <= N u d0, d0 the largest diagonal of B and u = 2^-53, and
 *                      the other N - r columns of L are exactly zero -- a lead with fewer open directions than rows is no error
 *     t = L_R^H (P_M L_L)                               two products on the FP64 matrix pipe, bracketed as written
 *     one-sided (Hestenes) Jacobi on the columns of t (of t^H when r_R < r_L: the zero columns stay columns): sweeps of N' - 1 rounds
 *     of N' / 2 disjoint pairs in the round-robin order, N' = 16, 32 or 64; a pair with a = |t_p|^2, b = |t_q|^2, c = t_p^H t_q is
 *     skipped when a == 0, b == 0 or |c| <= N u sqrt(a) sqrt(b), else rotated to orthogonality; the first sweep without a rotation
 *     is the last
 *     T_n = the squared column norms, descending; the entries beyond min(r_R, r_L) are exactly 0.0
 *
 * One-sided Jacobi keeps small T_n relatively accurate where an eigensolve of t^H t would bury them under u T_max.  The arguments, the
 * limits (n_s <= 4096, 256 MiB of staged devices), the groups and the errors are those of tbk_transmission_ensemble, with N <= 64
 * only: more rows are TBK_ERR_ARGUMENT, there is no library route.  Results: iterations int32 [nk][n_z] and T double
 * [nk][n_z][n_s], both with the bits of tbk_transmission_ensemble on the same input, and channels double [nk][n_z][n_s][N]; (N + 1)
 * doubles per (kp, z, sample) leave the device.  The bits of a channels[k][z][s] depend on nothing else: not on the groups, the
 * chunks, the grid, the other samples or their order.  A Jacobi that still rotates in its 48th sweep (the inputs of the tests need
 * 20 at most) is TBK_ERR_NO_CONVERGENCE; the message says that it was the channel iteration and names the k index, the energy and
 * the sample; a T_n that is not finite is TBK_ERR_SINGULAR with its sample, as a non-finite P_M is.  Error per T_n: (4 eps +
 * (2 (N + 1)^2 + 8 N (sweeps + 2) + N^2) u) scale / N with tbk_transmission's eps and scale. */

/* The kernel alone on principal layers the caller brings: tbk_transmission_ensemble_from_matrices' arguments.  k_chunk = 0: from the
 * size of the results, n_z n_s (8 N + 8) + 4 n_z bytes per point. */
int tbk_transmission_channels_from_matrices(int device, int N, int64_t n_k, const double* H00, const double* H01, int M, int64_t n_s, const double* V,
                                            const double* onsite, int64_t n_z, const double* z, int max_iterations, int64_t k_chunk,
                                            int64_t sample_chunk, int32_t* iterations, double* T, double* channels);
/* The whole call: k, layers, the chunks and H_m as in tbk_surface_green; the groups are chosen as for sample_chunk = 0.  Always the own
 * kernel, whatever TBK_OPT_EIGENSOLVER. */
int tbk_transmission_channels(tbk_model* m, int axis, int layers, const double* k, int64_t nk, int M, int64_t n_s, const double* V, const double* onsite,
                              int64_t n_z, const double* z, int max_iterations, int32_t* iterations, double* T, double* channels);
/* On several devices from one process: the slabs of tbk_hamilton_multi; every handle stages all the samples. */
int tbk_transmission_channels_multi(tbk_model* const* handles, int n_handles, int axis, int layers, const double* k, int64_t nk, int M, int64_t n_s,
                                    const double* V, const double* onsite, int64_t n_z, const double* z, int max_iterations, int32_t* iterations,
                                    double* T, double* channels);
/* ms[3] = the summed HIP-event time of H(k) with the principal layers, the decimation with the sweeps and the channels of every sample,
 * and the copies of the results to the host in this handle's calls made while TBK_OPT_TIMING was on; calls, reset as above.  A row of
 * its own: tbk_transmission_timing and tbk_transmission_ensemble_timing do not count these calls. */
int tbk_transmission_channels_timing(tbk_model* m, double* ms, int64_t* calls, int reset);

/* ---- the layer-resolved Green's functions of the device of tbk_transmission (not in the reference) -----------------------------------
 * H00, H01, N, L, V, M, the decimation and the forward sweep with g_p, D_p, T are those of tbk_transmission, unchanged down to the order
 * of the operations; Q_p below is its P_p.  Per (kp, z), after the forward sweep:
 *
 *     G_M = g_M,  C_M = g_M;   for p = M - 1 ... 1:  X = g_p H01,  Y = H01^H g_p,  G_p = g_p + (X G_{p+1}) Y,  C_p = X C_{p+1}
 *     F_1 = G_1,  F_p = G_p (H01^H Q_{p-1}) (1 < p < M),  F_M = Q_M (M > 1)
 *     ldos[p][i]  = -Im G_p[i][i] / pi
 *     left[p][i]  = Re sum_j (F_p Gamma_L)[i][j] conj(F_p[i][j]) / (2 pi)        right[p][i]: C_p and Gamma_R
 *
 * G_p, F_p and C_p are the blocks (p, p), (p, 1) and (p, M) of the resolvent of the device with both lead self-energies attached; left
 * and right are the parts of ldos injected from the two leads, and ldos - left - right = (Im z / pi) sum_q sum_j |G_pq[i][j]|^2.  Results:
 * iterations int32 [nk][n_z], T double [nk][n_z] (the bits of tbk_transmission), ldos, left, right double [nk][n_z][M][N] and, G, F and C
 * not NULL (all three or none), the blocks as double [nk][n_z][M][N][N][2].  The cap of the decimation is TBK_ERR_NO_CONVERGENCE; a zero
 * pivot or a non-finite element of any g_p, G_p, F_p or C_p is TBK_ERR_SINGULAR; the message names the first such k index and energy.
 * The bits of one (kp, z) depend on nothing else.  One workgroup owns a (kp, z) from the first decimation step to the last output; the
 * forward sweep leaves g_p and H01^H Q_{p-1} on a stack of 2 M N^2 complex numbers per workgroup, as many stacks as fit 1 GiB.  N <= 64:
 * there is no library route, and a handle with TBK_OPT_EIGENSOLVER = TBK_EIG_ROCSOLVER takes the own kernel as well.  H01 NULL,
 * layers = 0, M outside [1, 4096], V above 256 MiB, N > 64 and a stack above 1 GiB are TBK_ERR_ARGUMENT.
 * Error per component of a block B: eps c s, eps tbk_transmission's, c the number of error-carrying factors behind B and s the product of
 * the 2-norms of the blocks B is formed from. */

/* The kernel alone on principal layers the caller brings: H00, H01 double [n_k][N][N][2].  k_chunk: points per launch (0: from the size
 * of the results).  slots: a cap on the workgroups and their stacks (0: as many as fit). */
int tbk_device_green_from_matrices(int device, int N, int64_t n_k, const double* H00, const double* H01, int M, const double* V, int64_t n_z,
                                   const double* z, int max_iterations, int64_t k_chunk, int64_t slots, int32_t* iterations, double* T,
                                   double* ldos, double* left, double* right, double* G, double* F, double* C);
/* The whole call: k, layers, the chunks and H_m as in tbk_surface_green. */
int tbk_device_green(tbk_model* m, int axis, int layers, const double* k, int64_t nk, int M, const double* V, int64_t n_z, const double* z,
                     int max_iterations, int32_t* iterations, double* T, double* ldos, double* left, double* right, double* G, double* F,
                     double* C);
/* On several devices from one process: the slabs of tbk_hamilton_multi, every device writing its rows of the results. */
int tbk_device_green_multi(tbk_model* const* handles, int n_handles, int axis, int layers, const double* k, int64_t nk, int M, const double* V,
                           int64_t n_z, const double* z, int max_iterations, int32_t* iterations, double* T, double* ldos, double* left,
                           double* right, double* G, double* F, double* C);
/* ms[3] = the summed HIP-event time of H(k) with the principal layers, the decimation with both sweeps (one launch), and the copies of
 * the results to the host in this handle's calls made while TBK_OPT_TIMING was on; calls, reset as above. */
int tbk_device_green_timing(tbk_model* m, double* ms, int64_t* calls, int reset);

/* ---- the bond currents of the device of tbk_device_green (not in the reference) --------------------------------------------------------
 * Everything of tbk_device_green, unchanged down to the order of the operations, and with H_pp = H00 + V_p, per (kp, z):
 *
 *     A^L_{p,q} = (F_p Gamma_L) F_q^H            A^R_{p,q} = (C_p Gamma_R) C_q^H
 *     K^L_p[i][j] = 2 Im(conj(H01[i][j]) A^L_{p,p+1}[i][j])   p = 1 ... M - 1     from orbital i of layer p to orbital j of layer p + 1
 *     J^L_p[i][j] = 2 Im(conj(H_pp[i][j]) A^L_{p,p}[i][j])    p = 1 ... M         from orbital i to orbital j inside layer p
 *     K^R, J^R: the same with A^R;    current_left[p][i] = sum_j K^L_p[i][j],  current_right[p][i] = sum_j K^R_p[i][j]
 *
 * in e / h per unit energy: the currents of the states injected from the left and from the right lead.  sum_i current_left[p][i] tends
 * to T at every interface as Im z -> 0 and differs from the next interface's by 4 pi Im z sum_i left[p + 1][i]; K and J are exactly zero
 * where H01 and H_pp are.  Results: iterations, T, ldos, left, right as tbk_device_green, bit for bit; current_left, current_right double
 * [nk][n_z][M - 1][N]; and, the four bond arrays not NULL (all four or none), inter_left, inter_right (K) double [nk][n_z][M - 1][N][N] and
 * intra_left, intra_right (J) double [nk][n_z][M][N][N].  Without the bond arrays J is not formed.  A non-finite element of a K or J
 * that is formed is TBK_ERR_SINGULAR like one of a block.  The bits of one (kp, z) depend on nothing else, the bond arrays included.
 * The kernel is tbk_device_green's with four more products per layer (two without the bond arrays); F_p and C_p wait for the layer below
 * in the stack's places of g_p and H01^H Q_{p-1}, which are dead by then.  N <= 64; the argument errors are tbk_device_green's.
 * Error per component of K^L_p: 2 max|H01| (c(F_p) + c(F_{p+1}) + 1) eps s(F_p) s(F_{p+1}) 2 |H01|^2 |G_top|. */
int tbk_device_current_from_matrices(int device, int N, int64_t n_k, const double* H00, const double* H01, int M, const double* V, int64_t n_z,
                                     const double* z, int max_iterations, int64_t k_chunk, int64_t slots, int32_t* iterations, double* T,
                                     double* ldos, double* left, double* right, double* current_left, double* current_right, double* inter_left,
                                     double* inter_right, double* intra_left, double* intra_right);
int tbk_device_current(tbk_model* m, int axis, int layers, const double* k, int64_t nk, int M, const double* V, int64_t n_z, const double* z,
                       int max_iterations, int32_t* iterations, double* T, double* ldos, double* left, double* right, double* current_left,
                       double* current_right, double* inter_left, double* inter_right, double* intra_left, double* intra_right);
int tbk_device_current_multi(tbk_model* const* handles, int n_handles, int axis, int layers, const double* k, int64_t nk, int M, const double* V,
                             int64_t n_z, const double* z, int max_iterations, int32_t* iterations, double* T, double* ldos, double* left,
                             double* right, double* current_left, double* current_right, double* inter_left, double* inter_right,
                             double* intra_left, double* intra_right);
/* ms[3] as tbk_device_green_timing, of this handle's tbk_device_current calls. */
int tbk_device_current_timing(tbk_model* m, double* ms, int64_t* calls, int reset);

/* ---- the bare (Lindhard) static susceptibility of a uniform k mesh (not in the reference) ----------------------------------------
 * Mesh and mesh points k = (i_1 / n_1, ..., i_dim / n_dim) are those of tbk_occupations (dim 2 or 3); k+q is the mesh point with the
 * indices (i_d + q_d) mod n_d.  With E, U the eigenvalues and eigenvectors of tbk_eigh (convention 2), T = k_B T > 0 in the model's
 * energy units and the chemical potential mu (csrc/tbk_chi.hip):
 *     M(k, q)[b][b'] = sum_i conj(U[k][i][b]) D(q)[i] U[k+q][i][b']
 *     chi_0(q)       = -(1 / NK) sum_k sum_{b b'} F(E[k][b], E[k+q][b']) |M(k, q)[b][b']|^2
 *     F(a, b)        = (f(a) - f(b)) / (a - b),  F(a, a) = f'(a),  f(x) = 1 / (1 + exp((x - mu) / T))
 * D(q) = 1 for convention 2; for convention 1 D(q)[i] = exp(-2 pi i sum_d q_d pos[i][d] / n_d) with the unreduced q_d, a host table.
 * Without matrix elements |M|^2 = 1 and no eigenvector is computed.  F is evaluated as -f(lo) (1 - f(hi)) h(y) / T with lo <= hi,
 * y = (lo - hi) / T, h(y) = expm1(y) / y, h(0) = 1, f from exp(-|x - mu| / T) and 1 - f(x) as f(2 mu - x): no cancellation, no
 * overflow.  No spin factor; static only.  chi_0 >= 0, chi_0(-q) = chi_0(q); for given (E, U, mu, T) the bits of chi_0(q) depend on
 * q modulo the mesh and on D(q) alone -- not on the other vectors, their order, the batches or the number of handles -- and
 * repeated calls give the same bits.  |error| <= tol_chi of DESIGN.md 15.4.
 * q: int64 [n_q][dim] in mesh units, any value, duplicates allowed; chi_out: double [n_q].  The eigensystem of the WHOLE mesh stays
 * in device memory (NK n_orb^2 complex and 3 NK n_orb doubles; TBK_ERR_MEMORY, with the bytes in the message, when it does not
 * fit).  Argument errors (TBK_ERR_ARGUMENT), before any device is touched: those of tbk_occupations, T not finite or not positive,
 * n_q < 1, convention not in {1, 2}, convention 1 without pos, more than 16320 orbitals, more than 2^23 mesh points, a NULL
 * pointer.  Host buffers; synchronous. */

/* The kernels alone on an eigensystem the caller brings: E [NK][n_orb], U [NK][n_orb][n_orb] complex or NULL (no matrix elements),
 * phases: NULL or D [n_q][n_orb] complex (needs U). */
int tbk_chi_from_eigensystem(int device, int dim, const int32_t* mesh, int n_orb, const double* E, const double* U, double mu, double T,
                             int64_t n_q, const int64_t* q, const double* phases, double* chi_out);
/* The whole call: eigenvalues and mu (mode, value, mu_out as for tbk_occupations: mode 1 gives tbk_fermi's numbers bit for bit; the
 * finite-temperature chemical potential is not computed) through the slab route of tbk_occupations; then the handle fills the
 * resident eigensystem of the whole mesh chunk by chunk (tbk_eigh_device, whose own eigenvalues enter F; without matrix elements
 * the eigenvalue path), one kernel makes the Fermi tables, and the vectors go in batches of tbk_chi_plan's size through the overlap
 * kernel and the reduction.  pos: [n_orb][dim], read for convention 1. */
int tbk_susceptibility(tbk_model* m, const int32_t* mesh, int mode, double value, double T, int64_t n_q, const int64_t* q,
                       int matrix_elements, int convention, const double* pos, double* mu_out, double* chi_out);
/* On several devices from one process: mu from the slabs of tbk_occupations_multi; then every handle holds the whole mesh's
 * eigensystem and takes a contiguous share of the vectors (the first ceil(n_q / n_handles) to handle 0, ...). */
int tbk_susceptibility_multi(tbk_model* const* handles, int n_handles, const int32_t* mesh, int mode, double value, double T, int64_t n_q,
                             const int64_t* q, int matrix_elements, int convention, const double* pos, double* mu_out, double* chi_out);
/* How a call on nk mesh points, n_q vectors is run: out[0] = the overlap kernel's template (4: 64 x 64 blocks, 1: one tile, up to 16
 * orbitals, 0: no matrix elements), out[1] = partial sums per (k, q) pair, out[2] = vectors per batch when the partials may take
 * part_bytes (0: the library's budget of 256 MiB; at most 4096 vectors; 0 vectors: one does not fit), out[3] = batches. */
int tbk_chi_plan(int64_t nk, int n_orb, int64_t n_q, int matrix_elements, int64_t part_bytes, int64_t* out);
/* ms[3] = the summed HIP-event time of the Fermi tables, the overlaps with their epilogue (or the pair kernel), and the reduction
 * in this handle's calls made while TBK_OPT_TIMING was on; calls = how many calls; reset = 1 clears.  (The eigensolver stages are in
 * tbk_get_timing.) */
int tbk_chi_timing(tbk_model* m, double* ms, int64_t* calls, int reset);

/* ---- the bare dynamic susceptibility chi_0(q, omega + i eta) of a uniform k mesh (not in the reference) --------------------------
 * Mesh, k+q, q, E, U, D(q), matrix_elements, convention, mu (mode, value) and T are those of tbk_susceptibility.  With n_w real
 * frequencies omega_j (any sign and order, duplicates allowed) and one broadening eta > 0 (csrc/tbk_chi.hip):
 *     chi_0(q, z) = -(1 / NK) sum_k sum_{b b'} (f(E[k][b]) - f(E[k+q][b'])) / (E[k][b] - E[k+q][b'] + z) |M(k, q)[b][b']|^2,  z = omega + i eta
 * No spin factor; the sign is the static call's: Re chi_0(q, i eta) -> chi_0(q) as eta -> 0, less the f' terms of exactly degenerate
 * pairs, which the dynamic function does not have.  The occupation difference is evaluated as g = +-f(lo) (1 - f(hi)) (-expm1(y)),
 * lo <= hi, y = (lo - hi) / T, from the static call's tables, + where E[k][b] <= E[k+q][b'] (no cancellation, no overflow, a zero for
 * equal energies); per pair p = g |M|^2 and Delta = E[k][b] - E[k+q][b'] once, per frequency x = Delta + omega, r = 1 / (x^2 + eta^2),
 * Re -= p x r, Im += p eta r, over NK.  chi_0(-q, -omega + i eta) = conj chi_0(q, omega + i eta); for given (E, U, mu, T, eta) the
 * bits of chi_0(q, omega_j + i eta) depend on q modulo the mesh, D(q) and omega_j alone -- not on the other vectors or frequencies,
 * their order, the batches, the frequency passes or the number of handles -- and repeated calls give the same bits.  |error| of
 * either component <= the bound of DESIGN.md 16.4.
 * omega: double [n_w]; chi_out: [n_q][n_w] complex (Re, Im interleaved).  Argument errors (TBK_ERR_ARGUMENT), before any device is
 * touched: those of tbk_susceptibility, n_w < 1, more than 2^23 frequencies (one grid column of the reduction each), a NULL omega,
 * a frequency that is not finite, eta not finite or not positive (or so small that its square underflows to 0). */

/* The kernels alone on an eigensystem the caller brings (E, U, phases as for tbk_chi_from_eigensystem).  part_bytes: the bytes the
 * partial sums may take (0: the library's budget), as in tbk_chi_dynamic_plan. */
int tbk_chi_dynamic_from_eigensystem(int device, int dim, const int32_t* mesh, int n_orb, const double* E, const double* U, double mu, double T,
                                     int64_t n_q, const int64_t* q, const double* phases, int64_t n_w, const double* omega, double eta,
                                     int64_t part_bytes, double* chi_out);
/* The whole call: tbk_susceptibility's driver -- the same mu, the same resident eigensystem, the same wait on every exit -- with the
 * frequencies in device memory and the dynamic epilogue, pair kernel and reduction in place of the static ones. */
int tbk_dynamic_susceptibility(tbk_model* m, const int32_t* mesh, int mode, double value, double T, int64_t n_q, const int64_t* q, int64_t n_w,
                               const double* omega, double eta, int matrix_elements, int convention, const double* pos, double* mu_out,
                               double* chi_out);
/* On several devices from one process: tbk_susceptibility_multi's split, a contiguous share of the vectors (with all frequencies) per
 * handle. */
int tbk_dynamic_susceptibility_multi(tbk_model* const* handles, int n_handles, const int32_t* mesh, int mode, double value, double T,
                                     int64_t n_q, const int64_t* q, int64_t n_w, const double* omega, double eta, int matrix_elements,
                                     int convention, const double* pos, double* mu_out, double* chi_out);
/* How a call on nk mesh points, n_q vectors and n_w frequencies is run: out[0], out[1] as for tbk_chi_plan; the partial sums take
 * 16 nk out[1] bytes per (q, omega) and may take part_bytes (0: 256 MiB).  When all frequencies of one vector fit, out[4] = n_w,
 * out[5] = 1 and out[2] = vectors per batch (at most 4096), out[3] = batches; else out[2] = 1, out[3] = n_q and the frequencies go in
 * out[5] passes of out[4] (whole register chunks when one fits), the overlaps computed again in each.  out[2] = 0: not one (q, omega)
 * fits.  out[6] = the frequencies per register chunk of the epilogue.  out: int64 [7]. */
int tbk_chi_dynamic_plan(int64_t nk, int n_orb, int64_t n_q, int64_t n_w, int matrix_elements, int64_t part_bytes, int64_t* out);
/* (Kernel times of these calls are booked into tbk_chi_timing's three stages: the Fermi tables, the overlaps with the dynamic
 * epilogue or the dynamic pair kernel, the complex reduction; its call count includes them.) */

/* ---- the orbital-resolved bare static susceptibility chi_0[i][j](q) of a uniform k mesh (not in the reference) -----------------
 * Mesh, k+q, q, E, U, D(q), convention, mu (mode, value) and T are those of tbk_susceptibility; the eigenvectors are always used.
 * With t = f(lo) (1 - f(hi)) h(y) >= 0 of tbk_susceptibility (-T F) (csrc/tbk_chi.hip):
 *     A(k, q)[i; b, b'] = conj(U[k][i][b]) D(q)[i] U[k+q][i][b']
 *     chi_0[i][j](q)    = (1 / (T NK)) sum_k sum_{b b'} t(E[k][b], E[k+q][b']) A[i; b, b'] conj(A[j; b, b'])
 * No spin factor; static only; the sign is tbk_susceptibility's, whose chi_0(q) is the sum over (i, j).  chi_0(q) is Hermitian and
 * positive semidefinite, chi_0(-q) = chi_0(q)^T.  The output is exactly Hermitian: entries with i <= j (in ascending orbital order)
 * are computed, the others are their conjugates, the diagonal's imaginary part is +0.  m distinct orbitals are selected by
 * orbitals (int32 [m], any order; NULL with m = n_orb: all of them): chi_out is [n_q][m][m] complex (Re, Im interleaved) in the
 * caller's order, and every entry has the bits of the same entry of the full matrix.  For given (E, U, mu, T) the bits of an entry
 * depend on q modulo the mesh, D(q), i and j alone.  |error| per component <= chi_model.orbital_tolerance.
 * Argument errors (TBK_ERR_ARGUMENT), before any device is touched: those of tbk_susceptibility, m < 1 or m > n_orb, an index
 * out of range or repeated, a NULL orbitals with m != n_orb, a NULL output. */
/* The kernels alone on an eigensystem the caller brings (E, U, phases as for tbk_chi_from_eigensystem; U is required).  part_bytes:
 * the bytes the partial sums may take, k_slice: the k-points per slice (0: the library's own), as in tbk_chi_orbital_plan. */
int tbk_chi_orbital_from_eigensystem(int device, int dim, const int32_t* mesh, int n_orb, const double* E, const double* U, double mu, double T,
                                     int64_t n_q, const int64_t* q, const double* phases, int m, const int32_t* orbitals, int64_t part_bytes,
                                     int64_t k_slice, double* chi_out);
/* The whole call: tbk_susceptibility's driver -- the same mu, the same resident eigensystem, the same wait on every exit. */
int tbk_orbital_susceptibility(tbk_model* m, const int32_t* mesh, int mode, double value, double T, int64_t n_q, const int64_t* q, int n_sel,
                               const int32_t* orbitals, int convention, const double* pos, double* mu_out, double* chi_out);
/* On several devices from one process: tbk_susceptibility_multi's split, a contiguous share of the vectors per handle. */
int tbk_orbital_susceptibility_multi(tbk_model* const* handles, int n_handles, const int32_t* mesh, int mode, double value, double T,
                                     int64_t n_q, const int64_t* q, int m, const int32_t* orbitals, int convention, const double* pos,
                                     double* mu_out, double* chi_out);
/* How a call on nk mesh points, m of n_orb orbitals and n_q vectors is run: out[0] = the kernel's template (4: blocks of 64 x 64, four
 * waves; 1: one tile, m <= 16, a wave per slice), out[1] = blocks with i <= j per vector, out[2] = k-points per slice -- k_slice, or for
 * 0 the library's own, a function of (nk, n_orb) alone -- out[3] = slices, out[4] = vectors per batch (at most 4096; the partial sums
 * take 16 out[3] m'^2 bytes per vector, m' = m padded to the block, and may take part_bytes, 0: 256 MiB; 0: not one vector fits,
 * the call returns TBK_ERR_MEMORY), out[5] = batches.  out: int64 [6]. */
int tbk_chi_orbital_plan(int64_t nk, int n_orb, int m, int64_t n_q, int64_t part_bytes, int64_t k_slice, int64_t* out);
/* (Kernel times of these calls are booked into tbk_chi_timing's three stages: the Fermi tables, the rank-K update, the reduction of the
 * slices; its call count includes them.) */

/* ---- the orbital-resolved bare dynamic susceptibility chi_0[i][j](q, omega + i eta) of a uniform k mesh (not in the reference) ----
 * Mesh, k+q, q, E, U, D(q), convention, mu (mode, value) and T are those of tbk_susceptibility, omega, eta and z = omega + i eta those
 * of tbk_dynamic_susceptibility, A and the selection those of tbk_orbital_susceptibility (csrc/tbk_chi.hip):
 *     chi_0[i][j](q, z) = -(1 / NK) sum_k sum_{b b'} g(E[k][b], E[k+q][b']) / (E[k][b] - E[k+q][b'] + z) A[i; b, b'] conj(A[j; b, b'])
 * No spin factor; the sign is that of the other susceptibilities; the sum over (i, j) is tbk_dynamic_susceptibility's chi_0(q, z) with
 * matrix elements.  g and Delta = E[k][b] - E[k+q][b'] once per pair as there; per frequency x = Delta + omega, r = 1 / (x^2 + eta^2),
 * c = (g r x, -(g r eta)), X = c A, and chi = (0 - sum X conj(A)) / NK per component.  The matrix is NOT Hermitian: all m^2 entries are
 * computed.  chi_0[i][j](-q, -omega + i eta) = conj chi_0[i][j](q, omega + i eta).  For given (E, U, mu, T, eta) the bits of an entry
 * depend on q modulo the mesh, D(q), omega_j, i and j alone -- not on the other vectors, frequencies or selected orbitals, their order,
 * the batches, the frequency passes, the register chunk or the number of handles.  |error| per component <=
 * chi_model.dynamic_orbital_tolerance.
 * chi_out: [n_q][n_w][m][m] complex (Re, Im interleaved) in the caller's order of orbitals.  Argument errors (TBK_ERR_ARGUMENT), before
 * any device is touched: those of tbk_orbital_susceptibility and of tbk_dynamic_susceptibility, with at most 65535 frequencies per call
 * (one grid row of the reduction each). */
/* The kernels alone on an eigensystem the caller brings (E, U, phases as for tbk_chi_from_eigensystem; U is required).  part_bytes,
 * k_slice: as in tbk_chi_orbital_dynamic_plan. */
int tbk_chi_orbital_dynamic_from_eigensystem(int device, int dim, const int32_t* mesh, int n_orb, const double* E, const double* U, double mu,
                                             double T, int64_t n_q, const int64_t* q, const double* phases, int m, const int32_t* orbitals,
                                             int64_t n_w, const double* omega, double eta, int64_t part_bytes, int64_t k_slice,
                                             double* chi_out);
/* The whole call: tbk_susceptibility's driver -- the same mu, the same resident eigensystem, the same wait on every exit. */
int tbk_dynamic_orbital_susceptibility(tbk_model* m, const int32_t* mesh, int mode, double value, double T, int64_t n_q, const int64_t* q,
                                       int64_t n_w, const double* omega, double eta, int n_sel, const int32_t* orbitals, int convention,
                                       const double* pos, double* mu_out, double* chi_out);
/* On several devices from one process: tbk_susceptibility_multi's split, a contiguous share of the vectors (with all frequencies) per
 * handle. */
int tbk_dynamic_orbital_susceptibility_multi(tbk_model* const* handles, int n_handles, const int32_t* mesh, int mode, double value, double T,
                                             int64_t n_q, const int64_t* q, int64_t n_w, const double* omega, double eta, int m,
                                             const int32_t* orbitals, int convention, const double* pos, double* mu_out, double* chi_out);
/* How a call on nk mesh points, m of n_orb orbitals, n_q vectors and n_w <= 65535 frequencies is run: out[0] = the kernel's template
 * (as for tbk_chi_orbital_plan), out[1] = blocks per (q, omega): all nb^2 ordered ones, out[2] = k-points per slice -- k_slice, or for 0
 * the library's own, a function of (nk, n_orb) alone -- out[3] = slices, out[4] = frequencies per register chunk of the kernel.  The
 * partial sums take 16 out[3] m'^2 bytes per (q, omega), m' = m padded to the block, and may take part_bytes (0: 256 MiB).  When all
 * frequencies of one vector fit, out[7] = n_w, out[8] = 1, out[5] = vectors per batch (at most 4096, and as many as the grid takes with
 * their chunks) and out[6] = batches; else out[5] = 1, out[6] = n_q and the frequencies go in out[8] passes of out[7] (whole register
 * chunks when one fits), the update computed again in each.  out[5] = 0: not one (q, omega) fits, the call returns TBK_ERR_MEMORY.
 * out[9] = out[5] out[7], the (q, omega) per launch.  out: int64 [10]. */
int tbk_chi_orbital_dynamic_plan(int64_t nk, int n_orb, int m, int64_t n_q, int64_t n_w, int64_t part_bytes, int64_t k_slice, int64_t* out);
/* (Kernel times of these calls are booked into tbk_chi_timing's three stages: the Fermi tables, the complex-weighted rank-K update, the
 * reduction of the slices; its call count includes them.) */

/* ---- the four-index bare static susceptibility chi_0[i][l][j][m](q) of a uniform k mesh (not in the reference) ------------------
 * Mesh, k+q, q, E, U, mu (mode, value), T and t are those of tbk_orbital_susceptibility; convention 2 only: there is no phase table
 * (csrc/tbk_chi.hip):
 *     chi_0[i][l][j][m](q) = (1 / (T NK)) sum_k sum_{b b'} t(E[k][b], E[k+q][b'])
 *                            conj(U[k][i][b]) U[k+q][l][b'] U[k][j][b] conj(U[k+q][m][b'])
 * No spin factor; static only; the sign is tbk_susceptibility's.  chi_0[i][i][j][j] is tbk_orbital_susceptibility's chi_0[i][j].  As an
 * m^2 x m^2 matrix with rows (i, l) and columns (j, m) chi_0(q) is Hermitian and positive semidefinite, and the output is exactly
 * Hermitian: entries with (i, l) <= (j, m) (ascending orbital order, row-major pairs) are computed, the others are their conjugates
 * with the imaginary part formed as 0 - x, the diagonal's imaginary part is +0.  1 <= m <= 16 distinct orbitals are selected by
 * orbitals (int32 [m], any order; NULL with m = n_orb: all of them): chi_out is [n_q][m][m][m][m] complex (Re, Im interleaved) in
 * the caller's order, and every entry has the bits of the same entry of any other selection that holds its four orbitals.  For given
 * (E, U, mu, T) the bits of an entry depend on q modulo the mesh and its four orbitals alone.  |error| per component <=
 * chi_model.tensor_tolerance.
 * Argument errors (TBK_ERR_ARGUMENT), before any device is touched: those of tbk_orbital_susceptibility, and m > 16. */
/* The kernels alone on an eigensystem the caller brings (E, U as for tbk_chi_orbital_from_eigensystem; U is required).  part_bytes,
 * k_slice: as in tbk_chi_tensor_plan. */
int tbk_chi_tensor_from_eigensystem(int device, int dim, const int32_t* mesh, int n_orb, const double* E, const double* U, double mu, double T,
                                    int64_t n_q, const int64_t* q, int m, const int32_t* orbitals, int64_t part_bytes, int64_t k_slice,
                                    double* chi_out);
/* The whole call: tbk_susceptibility's driver -- the same mu, the same resident eigensystem, the same wait on every exit. */
int tbk_susceptibility_tensor(tbk_model* m, const int32_t* mesh, int mode, double value, double T, int64_t n_q, const int64_t* q, int n_sel,
                              const int32_t* orbitals, double* mu_out, double* chi_out);
/* On several devices from one process: tbk_susceptibility_multi's split, a contiguous share of the vectors per handle. */
int tbk_susceptibility_tensor_multi(tbk_model* const* handles, int n_handles, const int32_t* mesh, int mode, double value, double T,
                                    int64_t n_q, const int64_t* q, int m, const int32_t* orbitals, double* mu_out, double* chi_out);
/* How a call on nk mesh points, m <= 16 of n_orb orbitals and n_q vectors is run.  The kernel works on X[(i, j)][(l, m)] with the
 * m (m + 1) / 2 rows i <= j and the m^2 columns, in blocks of 64 x 64: out[0] = row blocks, out[1] = blocks per vector, out[2] =
 * k-points per slice -- k_slice, or for 0 the library's own, a function of (nk, n_orb) alone -- out[3] = slices, out[4] = vectors per
 * batch (at most 4096; the partial sums take 16 out[3] rows' cols' bytes per vector, rows and columns padded to 64, and may take
 * part_bytes, 0: 256 MiB; 0: not one vector fits, the call returns TBK_ERR_MEMORY), out[5] = batches.  out: int64 [6]. */
int tbk_chi_tensor_plan(int64_t nk, int n_orb, int m, int64_t n_q, int64_t part_bytes, int64_t k_slice, int64_t* out);
/* (Kernel times of these calls are booked into tbk_chi_timing's three stages: the Fermi tables, the two-stage kernel, the reduction of
 * the slices; its call count includes them.) */

/* ---- the lattice Berry flux and the Chern numbers of a uniform k mesh (not in the reference) -----------------------------------------
 * The Fukui-Hatsugai-Suzuki field strength (csrc/tbk_berry.hip, DESIGN.md section 18, tools/berry_model.py).  Mesh and mesh points are
 * those of tbk_occupations (dim 2 or 3), k+e_d is the mesh point with index (i_d + 1) mod n_d on axis d.  U is that of tbk_eigh
 * (convention 2); D(e_d) = 1 for convention 2 and exp(-2 pi i pos[i][d] / n_d) for convention 1 (the table of tbk_susceptibility for
 * q = e_d).  A band set is a half-open range [lo, hi) of band indices, m = hi - lo; a call takes 1 <= S <= 16 sets.  For every set,
 * axis d and mesh point k:
 *     M_d(k)     = U[k][:, lo:hi]^H D(e_d) U[k+e_d][:, lo:hi]                                  (m x m)
 *     L_d(k)     = det M_d(k)      LU with partial pivoting: the pivot is the largest |Re| + |Im|, a tie goes to the lowest row
 *     a_d(k)     = round(arg L_d(k) / (2 pi) 2^64) mod 2^64      the uint64 "angle word"; arg 0 = 0 for L = 0
 *     F_ab(k)    = a_a(k) + a_b(k+e_a) - a_a(k+e_b) - a_b(k)     wrapping 64-bit arithmetic, read as int64; a < b
 *     flux_ab(k) = (double)F_ab(k) 2 pi 2^-64                    in [-pi, pi]
 *     C_ab(i_c)  = (sum over the plane's k of F_ab(k)) / 2^64    an integer: the low word of the 128-bit sum is identically 0
 * Planes in the order (0,1), (0,2), (1,2); in two dimensions (0,1) alone.  C_ab is one integer per index i_c of the remaining axis c
 * (one per set in two dimensions).  Only the link angles carry rounding; what follows them is integer arithmetic, so the Chern
 * numbers are integers whatever the eigensolver's gauge.  The bits of a link depend on U(k), U(k+e_d), D, lo and hi alone -- not on the
 * other sets, the batch or the handle.  Angle error per link <= berry_model.link_tolerance.
 * Argument errors (TBK_ERR_ARGUMENT), before any device is touched: those of tbk_occupations' mesh, n_sets outside [1, 16], lo < 0,
 * hi > n_orb or lo >= hi, convention not in {1, 2}, convention 1 without pos, a NULL pointer, a k.p handle, a handle given twice.
 * Host buffers; synchronous. */

/* The link kernels alone on eigenvectors the caller brings: U [NK][n_orb][n_orb] complex, ranges int32 [n_sets][2], phases NULL or
 * D [dim][n_orb] complex; L_out complex [n_sets][dim][NK], words_out uint64 of the same shape. */
int tbk_berry_links_from_eigensystem(int device, int dim, const int32_t* mesh, int n_orb, const double* U, int n_sets, const int32_t* ranges,
                                     const double* phases, double* L_out, uint64_t* words_out);
/* The plaquette kernel alone on words the caller brings: words uint64 [n_sets][dim][NK]; flux_out double [n_sets][P][NK] (P = 1 or 3
 * planes), chern_out int64 [n_sets][sum of n_c over the planes] (n_2 + n_1 + n_0 in three dimensions, 1 in two). */
int tbk_berry_flux_from_links(int device, int dim, const int32_t* mesh, int n_sets, const uint64_t* words, double* flux_out,
                              int64_t* chern_out);
/* The whole call: the handle fills the resident eigenvectors of the whole mesh chunk by chunk as tbk_susceptibility does (the same
 * workspaces, the same routine), then the links, then the fluxes.  No chemical potential.  link_min_out: double [n_sets], the smallest
 * |L_d(k)| of each set (small: the mesh is too coarse or the set is not isolated). */
int tbk_berry_flux(tbk_model* m, const int32_t* mesh, int n_sets, const int32_t* ranges, int convention, const double* pos,
                   double* flux_out, int64_t* chern_out, double* link_min_out);
/* On several devices from one process: every handle holds the whole mesh's eigenvectors and computes the links of a contiguous share
 * of the mesh points (the first ceil(NK / n_handles) to handle 0, ...); the host concatenates the words and handle 0 runs the plaquette
 * kernel.  The number of handles changes no bit. */
int tbk_berry_flux_multi(tbk_model* const* handles, int n_handles, const int32_t* mesh, int n_sets, const int32_t* ranges, int convention,
                         const double* pos, double* flux_out, int64_t* chern_out, double* link_min_out);
/* How the links of nk mesh points are computed, per set: out[2 s] = the template (1: m <= 16, a link per wave, LU in the wave; 4:
 * m <= 64, a link per workgroup, LU in LDS; 64: m > 64, the product kernel writes M and rocsolver_zgetrf_strided_batched factors it),
 * out[2 s + 1] = links per launch at most (never more than the 3 nk links a set can have).  out: int64 [2 n_sets]. */
int tbk_berry_plan(int64_t nk, int n_orb, int n_sets, const int32_t* ranges, int64_t* out);
/* ms[3] = the summed HIP-event time of the link kernels (the products of the library path included), the library's LU with the
 * determinant kernel, and the plaquette kernel in this handle's calls made while TBK_OPT_TIMING was on; calls = how many calls;
 * reset = 1 clears.  (The eigensolver stages are in tbk_get_timing.) */
int tbk_berry_timing(tbk_model* m, double* ms, int64_t* calls, int reset);

/* ---- the Kubo optical conductivity sigma[a][c](omega + i eta) of a uniform k mesh (not in the reference) --------------------------
 * Mesh, mu (mode, value), T, the frequencies omega[n_w] and eta are those of tbk_dynamic_susceptibility; dim is 2 or 3.  With E, U of
 * tbk_eigh (convention 2) at the mesh points, D^a(k) = (1 / 2 pi) dH/dk_a = sum_R i R_a exp(2 pi i k.R) hop[R] + h.c. and
 * V^a = U^H D^a U -- for convention 1 plus i (E_b - E_b') (U^H diag(pos[:, a]) U)[b][b'], pos[n_orb][dim] --
 *
 *     sigma[a][c](omega) = (i / NK) sum_k sum_{b b'} w V^a[b][b'] conj(V^c[b][b']) / (omega + i eta + E_b - E_b'),
 *     w = -(f(E_b) - f(E_b')) / (E_b - E_b') >= 0, -f' on equal energies, evaluated as T F of tbk_susceptibility is.
 *
 * sigma_out: complex [n_w][dim][dim] in reduced coordinates, e = hbar = 1, per unit cell, no spin factor; mu_out: double [4] as for
 * tbk_susceptibility.  The mesh is walked in chunks of eigenvectors; the velocity matrices never leave the device.  The bits of
 * sigma(omega_j) do not depend on the other frequencies, their order or part_bytes: per-k partial sums are added in groups of 256
 * consecutive mesh points in index order, the groups in index order, and handles take whole groups.  They do not depend on
 * TBK_OPT_K_CHUNK or the number of handles either for sparse models and for dense models on the matrix-vector H(k) kernel (at most
 * 256 padded packed slots, i.e. up to 22 orbitals, and fewer than 128 lattice vectors): their walk stays in chunks of at most 4096
 * points, which all run one arithmetic.  For a larger dense model the eigensystem and D^a of a k-point are those of the H(k) kernel
 * its chunk takes (matrix-vector up to 32 points, tiles split along K by the number of tiles above), which differ in the last bit
 * with the chunk's length, as tbk_eigh's do; the sums add nothing to that.  part_bytes: the bytes the partial sums of one pass over
 * the mesh may take (0: the library's budget, 1 GiB or a quarter of the device's free memory if that is less); tbk_optics_plan. */
int tbk_optical_conductivity(tbk_model* m, const int32_t* mesh, int mode, double value, double T, int64_t n_w, const double* omega,
                             double eta, int convention, const double* pos, int64_t part_bytes, double* mu_out, double* sigma_out);
int tbk_optical_conductivity_multi(tbk_model* const* handles, int n_handles, const int32_t* mesh, int mode, double value, double T,
                                   int64_t n_w, const double* omega, double eta, int convention, const double* pos,
                                   int64_t part_bytes, double* mu_out, double* sigma_out);
/* The kernels on the caller's arrays (tests): E[nk][n_orb], U[nk][n_orb][n_orb] complex, D[nk][dim][n_orb][n_orb] complex (Hermitian),
 * pos NULL or [n_orb][dim]; all nk points are one chunk. */
int tbk_optics_from_eigensystem(int device, int dim, int n_orb, int64_t nk, const double* E, const double* U, const double* D,
                                const double* pos, double mu, double T, int64_t n_w, const double* omega, double eta,
                                int64_t part_bytes, double* sigma_out);
/* How a call on nk mesh points and n_w frequencies is run: out[0] = the fused kernel's template (the orbitals padded to 16, 32 or 64;
 * 0: above 64 orbitals, the products go through rocBLAS), out[1] = the frequencies per register chunk of the epilogue, out[2] = the
 * frequencies per pass when the partial sums (16 dim^2 nk bytes per frequency) may take part_bytes (0: 1 GiB -- a call on a device
 * with less than 4 GiB free takes a quarter of the free memory instead, so pass that figure to see its passes; whole register chunks
 * when one fits; 0: not one frequency fits, the call returns TBK_ERR_MEMORY), out[3] = passes, every one of which walks the mesh
 * again, out[4] = summation groups of 256 mesh points.  out: int64 [5]. */
int tbk_optics_plan(int64_t nk, int n_orb, int dim, int64_t n_w, int64_t part_bytes, int64_t* out);
/* ms[3] = the summed HIP-event time of the derivative H(k) contractions, the rotation into the band basis with its epilogue (the
 * Fermi tables and the library route's products included), and the reductions in this handle's calls made while TBK_OPT_TIMING was
 * on; calls = how many calls; reset = 1 clears.  (The eigensolver stages are in tbk_get_timing.) */
int tbk_optics_timing(tbk_model* m, double* ms, int64_t* calls, int reset);
/* D^a = (1 / 2 pi) dH/dk_a of nk k-points on device buffers, FULL, convention 2, axis in [0, dim): d_D [nk][n_orb][n_orb] complex.
 * The H(k) kernels on derivative phase rows (-R_a sin, +R_a cos) with the staged operand; a test hook, enqueued only. */
int tbk_hamilton_derivative_device(tbk_model* m, const double* d_k, int64_t nk, int axis, double* d_D);

/* ---- the transport distribution Sigma[a][c](E) of a uniform k mesh by the tetrahedron method (not in the reference) ---------------
 * mesh, the energy grid (e_min, e_step, n_e), the simplices, the half-open ranges and the stable sort are those of tbk_dos /
 * tbk_pdos; dim is 2 or 3.  With E, U of tbk_eigh (convention 2) at the mesh points, D^a = (1 / 2 pi) dH/dk_a and V^a = U^H D^a U,
 *
 *     w[a][c](k, b) = Re sum_{b' : fabs(E_b - E_b') <= degeneracy} V^a[b][b'] conj(V^c[b][b'])       (v_a v_c of an isolated band)
 *
 * is integrated by Bloechl's corner weights as tbk_pdos integrates A_g, through G = dim (dim + 1) / 2 non-negative channels: channel
 * a < dim is sum |V^a|^2, channel dim + p is sum |V^a + V^c|^2 for the pairs a < c in the order (0, 1), (0, 2), (1, 2).
 * cumulative_out: double [G][n_e], channel g integrated up to every grid energy, per unit cell, reduced coordinates, e = hbar = 1, no
 * spin factor; N[a][c] = (N+[a][c] - N[a][a] - N[c][c]) / 2 is the caller's step.  scale: double [G], positive and finite: the
 * kernels divide channel g by scale[g] so that the fixed point of tbk_pdos receives weights in [0, 1], and the result is multiplied
 * back -- exactly, and with bits that do not depend on the handles, when the scales are powers of two.  scale[g] must bound the
 * channel's weights: the next power of two above 1.0000001 B_a^2, or (B_a + B_c)^2, B_a = sum_R |R_a| ||hop[R]||_F over both halves
 * of the lattice, does.  A weight above scale[g] is counted, never clamped: the call fails with TBK_ERR_ARGUMENT and names the channel.
 * For given scales the bits depend neither on a second call nor, for sparse models and dense models on the matrix-vector H(k)
 * kernel, on TBK_OPT_K_CHUNK or the number of handles (the walk is tbk_optical_conductivity's).  Argument errors
 * (TBK_ERR_ARGUMENT), before any device is touched: those of tbk_dos, degeneracy negative or not finite, a scale that is not positive
 * and finite, a k.p handle, a handle given twice. */
int tbk_transport_distribution(tbk_model* m, const int32_t* mesh, double e_min, double e_step, int64_t n_e, double degeneracy,
                               const double* scale, double* cumulative_out);
int tbk_transport_distribution_multi(tbk_model* const* handles, int n_handles, const int32_t* mesh, double e_min, double e_step,
                                     int64_t n_e, double degeneracy, const double* scale, double* cumulative_out);
/* The weights kernels on the caller's arrays (tests): E[nk][n_orb], U[nk][n_orb][n_orb] complex, D[nk][dim][n_orb][n_orb] complex; all
 * nk points are one chunk.  W_out: double [nk][G][n_orb], the channels divided by their scales. */
int tbk_tdf_weights_from_eigensystem(int device, int dim, int n_orb, int64_t nk, const double* E, const double* U, const double* D,
                                     double degeneracy, const double* scale, double* W_out);
/* ms[3] = the summed HIP-event time of the derivative H(k) contractions, the weights kernel (the library route's products included),
 * and accumulate + reduction + scan in this handle's calls made while TBK_OPT_TIMING was on; calls = how many calls; reset = 1
 * clears.  (The eigensolver stages are in tbk_get_timing.) */
int tbk_tdf_timing(tbk_model* m, double* ms, int64_t* calls, int reset);

/* ---- k.p models (kdotp.py:51-100): H(k) = sum_p prod_d k_d^powers[p][d] * coeffs[p] ------- */
int tbk_kdotp_create(int device, int dim, int n_orb, int64_t n_p, const int32_t* powers,
                     const double* coeffs, tbk_kdotp** out);
void tbk_kdotp_destroy(tbk_kdotp* m);
int tbk_kdotp_hamilton(tbk_kdotp* m, const double* k, int64_t nk, double* H_out);
int tbk_kdotp_eigenval(tbk_kdotp* m, const double* k, int64_t nk, double* E_out);
int tbk_kdotp_eigh(tbk_kdotp* m, const double* k, int64_t nk, double* E_out, double* U_out);  /* tbk_eigh, convention 2 */
/* The same on several devices from one process: staged copies of ONE k.p model, contiguous k slabs, one host thread
 * per non-empty slab -- tbk_eigenval_multi / tbk_hamilton_multi for kdotp.py:51-100. */
int tbk_kdotp_eigenval_multi(tbk_kdotp* const* handles, int n_handles, const double* k, int64_t nk, double* E_out);
int tbk_kdotp_hamilton_multi(tbk_kdotp* const* handles, int n_handles, const double* k, int64_t nk, double* H_out);
int tbk_kdotp_eigh_multi(tbk_kdotp* const* handles, int n_handles, const double* k, int64_t nk, double* E_out, double* U_out);

/* Model.construct_kdotp (_tb_model.py:942-982): Taylor coefficients of H(k) around k0 for n_p power
 * tuples.  powers: int32 [n_p][dim]; prefactor: double [n_p][2] = (2 pi i)^{|p|} / prod p_d! as (re, im);
 * coeffs_out: double [n_p][n_orb][n_orb][2] (Hermitian matrices).  Host buffers; dense handles only. */
int tbk_kdotp_coefficients(tbk_model* m, const double* k0, int64_t n_p, const int32_t* powers,
                           const double* prefactor, double* coeffs_out);

/* ---- device memory helpers (so a Python host needs no other GPU runtime) ----------------- */
int tbk_device_malloc(int device, int64_t bytes, void** d_ptr);
int tbk_device_free(int device, void* d_ptr);
int tbk_memcpy_h2d(int device, void* d_dst, const void* h_src, int64_t bytes);
int tbk_memcpy_d2h(int device, void* h_dst, const void* d_src, int64_t bytes);
int tbk_device_mem_info(int device, int64_t* free_bytes, int64_t* total_bytes);

/* ---- timing: HIP events around every kernel of the path, on the stream it is launched on -------
 * stages: PHASE phase rows; HK the H(k) contraction; EIG reduction to tridiagonal form (or the whole
 * rocSOLVER call, and the eigenvector solver of tbk_eigh); QL the tridiagonal stage (QL + sort, or bisection).  Stages of different k chunks may overlap. */
enum { TBK_T_PHASE = 0, TBK_T_HK = 1, TBK_T_EIG = 2, TBK_T_QL = 3, TBK_T_COUNT = 4 };
/* ms[i] = summed duration of stage i, launches[i] = number of timed launches; reset = 1 clears. */
int tbk_get_timing(tbk_model* m, double* ms, int64_t* launches, int reset);

/* ---- multi-GPU: one process per GPU, RCCL over xGMI --------------------------------------- */
/* 128-byte RCCL unique id, created on rank 0 and handed to the other ranks by the launcher. */
int tbk_comm_unique_id(void* id128);
int tbk_comm_create(int device, int world_size, int rank, const void* id128, tbk_comm** out);
void tbk_comm_destroy(tbk_comm* c);
/* Size of the communicator and this process' rank in it, as RCCL reports them (ncclCommCount / ncclCommUserRank). */
int tbk_comm_ranks(tbk_comm* c, int* count, int* rank);
/* All-gather of per-rank eigenvalue slabs: every rank contributes `count` doubles from d_send and
 * receives world_size * count doubles in rank order in d_recv.  Enqueued on `m`'s stream; with m == NULL (a rank
 * that could not stage its model still has to take part) on the communicator's own stream (tbk_comm_synchronize). */
int tbk_comm_allgather_f64(tbk_comm* c, tbk_model* m, const double* d_send, double* d_recv,
                           int64_t count);
/* The same gather on the communicator's own stream: it starts once the work enqueued on `m`'s stream so far
 * is complete and overlaps whatever is enqueued on `m` afterwards.  Callers alternate two (send, recv) pairs,
 * slot 0 / 1; tbk_comm_wait_slot makes `m`'s stream wait for the previous gather of a slot before its buffers
 * are written again (stream dependency, the host does not block); tbk_comm_synchronize waits on the host. */
int tbk_comm_allgather_f64_overlapped(tbk_comm* c, tbk_model* m, const double* d_send, double* d_recv,
                                      int64_t count, int slot);
int tbk_comm_wait_slot(tbk_comm* c, tbk_model* m, int slot);
int tbk_comm_synchronize(tbk_comm* c);
/* Agreement in front of a sharded call: every rank contributes `status` (0 = ready to take part), verdict[world]
 * (HOST) receives every rank's word.  One 8-byte all-gather through buffers the communicator owns since its
 * creation; synchronous.  A rank whose staging / allocation failed reports it HERE, and nobody enters the data
 * collectives (a rank raising alone in front of a collective leaves its peers hanging in it). */
int tbk_comm_agree(tbk_comm* c, int status, double* verdict);
/* The landing area of tbk_eigenval_device_gather for slabs of `per` rows of n_orb eigenvalues (grow-only, sized from per,
 * n_orb and the world size alone).  Call it in the step whose outcome tbk_comm_agree exchanges: an allocation failure on one
 * rank then reaches every rank's verdict BEFORE anybody enters the data collectives.  (The gather allocates by itself when
 * this was skipped; a failure there travels in that rank's status word, behind the same sequence of collectives.) */
int tbk_comm_prepare_gather(tbk_comm* c, int n_orb, int64_t per);

/* One sharded eigenvalue call with the gather pipelined behind the k chunks (replaces the per-process body of a
 * multiprocessing farm over Model.eigenval, _tb_model.py:1134-1150; k-points are independent, :1111-1123).
 * Every rank calls it with the SAME `per` (slab length in k-points = ceil(NK / world)) and its own nk <= per k-points
 * (d_k / h_k as in tbk_eigenval_device_hint).  d_all[world][per][n_orb] (device) receives the eigenvalues of ALL ranks in
 * rank = caller order: this rank's rows are computed in place, and while later k chunks compute, finished blocks of
 * rows are all-gathered on the communicator's stream and moved to their places; rows nk..per of a short slab are
 * zero.  host_status != 0: this rank computes nothing and reports that status (a failure in front of the call).
 * d_status_all[world] (device) receives every rank's tbk_status as doubles (the solvers' non-finite / convergence
 * flags included; they are consumed) -- the last collective of the call, so every rank sees the same verdict.
 * Everything is enqueued: tbk_comm_synchronize(c) waits for the result, and `m`'s main stream waits for the gathers
 * before any later call touches the buffers. */
int tbk_eigenval_device_gather(tbk_comm* c, tbk_model* m, const double* d_k, const double* h_k, int64_t nk, int64_t per,
                               int host_status, double* d_all, double* d_status_all);

/* ---- microbenchmark: sustained v_mfma_f64_16x16x4_f64 rate of the device (TFLOP/s) -------- */
int tbk_mfma_f64_peak(int device, double* tflops);

#ifdef __cplusplus
}
#endif
#endif /* TBK_H */
