// tbk_api.hip -- the C ABI of include/tbk.h: staging, the chunked k pipeline, host/device entry
// points.  Kernels live in tbk_phase.hip / tbk_stage.hip / tbk_hk_dense.hip / tbk_hk_csr.hip, the
// eigensolver's in tbk_eig_small.hip / tbk_eig_stream.hip / tbk_eig_band*.hip (tbk_eig.hip: the rocSOLVER
// path), and which of them a call takes is tbk_eig_plan's (tbk_eig_plan.hip); a k list that folds is driven by
// tbk_folded_call (tbk_fold.hip), which hands the pipeline here its H(k) builder.  This file only owns memory, streams
// and ordering.  What belongs to one call (tbk_one_k_t, the gather's chunk hook) travels down as arguments: the handle holds none.

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <functional>
#include <new>
#include <vector>

#include "tbk_internal.h"

// ------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------
static thread_local char g_err[1024] = "";

void tbk_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* tbk_last_error(void) { return g_err; }
extern "C" const char* tbk_version(void) { return "tbk 0.1 (gfx950)"; }

extern "C" int tbk_device_count(int* count) {
    TBK_ARG(count != nullptr, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        n = 0;
    }
    *count = n;
    return TBK_OK;
}

// ------------------------------------------------------------------------------------------------
// helpers
// ------------------------------------------------------------------------------------------------
int DevBuf::reserve(size_t want) {
    if (want <= bytes) return TBK_OK;
    bytes = 0;
    const size_t rounded = (want + (size_t(1) << 20) - 1) & ~((size_t(1) << 20) - 1);
    TBK_HIP(hipMalloc(ptr.put(), rounded));
    bytes = rounded;
    return TBK_OK;
}

void SpanRecorder::start(int stage) {
    if (!on) return;
    EventSpan span;
    span.stage = stage;
    if (hipEventCreate(span.start.put()) != hipSuccess || hipEventCreate(span.stop.put()) != hipSuccess) {
        (void)hipGetLastError();
        on = false;
        return;
    }
    (void)hipEventRecord(span.start, stream);
    spans.push_back(std::move(span));
}

void SpanRecorder::stop() {
    if (on && !spans.empty()) (void)hipEventRecord(spans.back().stop, stream);
}

void SpanRecorder::collect(double* ms) {
    std::vector<float> t(spans.size(), 0.f);
    for (size_t i = 0; i < spans.size() && on; ++i)
        if (hipEventElapsedTime(&t[i], spans[i].start, spans[i].stop) != hipSuccess) on = false;
    for (size_t i = 0; i < spans.size() && on; ++i) ms[spans[i].stage] += (double)t[i];
    spans.clear();
}

int tbk_timed_read(tbk_model* m, TimedFamily family, int stages, double* ms, int64_t* calls, int64_t* passes, int reset) {
    TBK_LOCK(m);
    TimedSums& row = m->timed[family];
    for (int i = 0; i < stages; ++i) ms[i] = row.ms[i];
    *calls = row.calls;
    if (passes) *passes = row.passes;
    if (reset) row = TimedSums();
    return TBK_OK;
}

// roctx ranges (rocprofv3 --marker-trace labels the timeline with them): the tools library is looked up at run time,
// so libtbk.so has no link-time dependency on it; ranges are only pushed while TBK_OPT_TIMING is on.
namespace {
struct RoctxApi {
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
};
const RoctxApi& roctx_api() {
    static const RoctxApi api = [] {
        RoctxApi a;
        for (const char* name : {"librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so"}) {
            void* h = dlopen(name, RTLD_LAZY | RTLD_GLOBAL);
            if (!h) continue;
            a.push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
            a.pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
            if (a.push && a.pop) break;
            a.push = nullptr;
            a.pop = nullptr;
        }
        return a;
    }();
    return api;
}
const char* const kStageNames[TBK_T_COUNT] = {"tbk:phase_rows", "tbk:hk_contraction", "tbk:tridiag_reduction",
                                              "tbk:tridiag_eigenvalues"};
}  // namespace

void tbk_range_push(const char* name) {
    const RoctxApi& api = roctx_api();
    if (api.push) (void)api.push(name);
}

void tbk_range_pop() {
    const RoctxApi& api = roctx_api();
    if (api.pop) (void)api.pop();
}

StageTimer::StageTimer(tbk_model* m_, int stage, hipStream_t s)
    : m(m_), on(m_->timing), stream(s ? s : m_->stream) {
    ev.stage = stage;
    if (on) {
        if (hipEventCreate(ev.start.put()) != hipSuccess || hipEventCreate(ev.stop.put()) != hipSuccess) {
            on = false;
            return;
        }
        tbk_range_push(kStageNames[stage]);
        (void)hipEventRecord(ev.start, stream);
    }
}

StageTimer::~StageTimer() {
    if (on) {
        (void)hipEventRecord(ev.stop, stream);
        tbk_range_pop();
        m->events.push_back(std::move(ev));
    }
}

static inline int64_t round_up(int64_t x, int64_t q) { return (x + q - 1) / q * q; }

static int require_device(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) {
        (void)hipGetLastError();
        tbk_set_error("no HIP device visible: libtbk has no CPU path");
        return TBK_ERR_DEVICE;
    }
    if (device < 0 || device >= n) {
        tbk_set_error("device %d out of range (have %d)", device, n);
        return TBK_ERR_ARGUMENT;
    }
    TBK_HIP(hipSetDevice(device));
    return TBK_OK;
}

// a handle under construction: destroyed on every early return, released into *out on success
struct ModelDestroy {
    void operator()(tbk_model* m) const { tbk_model_destroy(m); }
};
using ModelGuard = std::unique_ptr<tbk_model, ModelDestroy>;

// everything both model kinds share: stream, rocBLAS handle, lattice vectors, packed-element map
// (pair_diagonal: the slot map of dense tight-binding models, two diagonal elements per slot -- tbk_internal.h)
static int create_common(int device, int dim, int n_orb, int64_t n_r, const int32_t* R,
                         int64_t k_rows_per_r, bool pair_diagonal, ModelGuard* out) {
    TBK_ARG(dim >= 1 && dim <= TBK_MAX_DIM, "dim must be in [1, 8]");
    TBK_ARG(n_orb >= 1 && n_orb <= 32768, "n_orb must be in [1, 32768]");
    TBK_ARG(n_r >= 0 && n_r < (int64_t(1) << 28), "n_r out of range");
    TBK_ARG(n_r == 0 || R != nullptr || k_rows_per_r == 1, "R is NULL");  // k.p rows carry no R
    TBK_CHECK(require_device(device));

    ModelGuard guard(new (std::nothrow) tbk_model());
    tbk_model* m = guard.get();
    if (!m) {
        tbk_set_error("out of host memory");
        return TBK_ERR_MEMORY;
    }
    m->device = device;
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) m->n_cu = cus;
    }
    m->dim = dim;
    m->n_orb = n_orb;
    m->n_r = n_r;
    // K rows are padded to whole LDS stages (TBK_BK); padding rows carry zero hoppings.  Dense tight-binding models large enough
    // for the Strassen path (tbk_internal.h) pad to whole stages in each HALF of K and to whole element tiles in each half of
    // the slots (padding slots keep colmap -1)
    const bool strassen = pair_diagonal && k_rows_per_r == 2 && tbk_strassen_model(false, false, n_r);
    m->k2 = round_up(n_r * k_rows_per_r, strassen ? 2 * TBK_BK : TBK_BK);
    m->n_r_pad = m->k2 / k_rows_per_r;
    m->ncol = (int)(pair_diagonal ? (int64_t)n_orb * (n_orb - 1) / 2 + (n_orb + 1) / 2 : (int64_t)n_orb * (n_orb + 1) / 2);
    m->ncol_pad = (int)round_up(m->ncol, strassen ? 2 * TBK_BNP : TBK_BNP);

    TBK_HIP(hipStreamCreateWithFlags(m->stream.put(), hipStreamNonBlocking));
    TBK_HIP(hipStreamCreateWithFlags(m->stream_eig.put(), hipStreamNonBlocking));
    TBK_HIP(hipStreamCreateWithFlags(m->stream_ql.put(), hipStreamNonBlocking));
    // (stream_xl / ev_xl: created by launch_band_xl when a batch above 1024 orbitals first goes in groups)
    for (int b = 0; b < 2; ++b) {
        TBK_HIP(hipEventCreateWithFlags(m->ev_hk[b].put(), hipEventDisableTiming));
        TBK_HIP(hipEventCreateWithFlags(m->ev_tri[b].put(), hipEventDisableTiming));
        TBK_HIP(hipEventCreateWithFlags(m->ev_ql[b].put(), hipEventDisableTiming));
        TBK_HIP(hipEventCreateWithFlags(m->ev_out[b].put(), hipEventDisableTiming));
        TBK_HIP(hipEventCreateWithFlags(m->ev_s2[b].put(), hipEventDisableTiming));
        // (release to system scope: results of small calls are read by the CPU from non-coherent pinned memory right
        // behind hipEventSynchronize on this event -- with a default event that visibility is the runtime's choice)
        if (b == 0) TBK_HIP(hipEventCreateWithFlags(m->ev_sync.put(), hipEventDisableTiming | hipEventReleaseToSystem));
    }
    TBK_ROCBLAS(rocblas_create_handle(m->blas.put()));
    TBK_ROCBLAS(rocblas_set_stream(m->blas, m->stream));
    TBK_CHECK(m->ws_flag.reserve(2 * sizeof(int)));
    TBK_HIP(hipMemsetAsync(m->ws_flag.ptr, 0, 2 * sizeof(int), m->stream));
    // one H(k) (up to 1024 orbitals: 16 MiB) with its k-point and positions, or a few hundred eigenvalue rows
    m->h_stage_bytes = std::max<size_t>(size_t(320) << 10,
                                        n_orb <= 1024 ? (size_t)n_orb * n_orb * 16 + (size_t)n_orb * dim * 8 + (size_t(64) << 10) : 0);
    if (hipHostMalloc(m->h_stage.put(), m->h_stage_bytes, hipHostMallocNonCoherent) != hipSuccess) {
        (void)hipGetLastError();
        m->h_stage.h = nullptr;  // no pinned memory: every call takes the pageable path
        m->h_stage_bytes = 0;
    }

    // packed upper-triangle map, row-major over (i <= j): consecutive e -> consecutive j.  With pair_diagonal, row i
    // starts with the slot of the diagonal pair (i, i + 1) when i is even (a single (i, i) for the last row of an odd
    // n_orb, whose Im plane is then 0 by construction) and holds no diagonal slot when i is odd.
    {
        std::vector<int32_t> colmap((size_t)m->ncol_pad, -1);
        size_t e = 0;
        for (int i = 0; i < n_orb; ++i) {
            if (!pair_diagonal)
                colmap[e++] = (int32_t)((i << 16) | i);
            else if (i % 2 == 0)
                colmap[e++] = i + 1 < n_orb ? (int32_t)((i << 16) | TBK_SLOT_PAIR | (i + 1)) : (int32_t)((i << 16) | i);
            for (int j = i + 1; j < n_orb; ++j) colmap[e++] = (int32_t)((i << 16) | j);
        }
        TBK_HIP(hipMalloc(m->d_colmap.put(), colmap.size() * sizeof(int32_t)));
        TBK_HIP(hipMemcpy(m->d_colmap, colmap.data(), colmap.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        m->staged_bytes += (int64_t)(colmap.size() * sizeof(int32_t));
    }
    if (n_r > 0 && R != nullptr && k_rows_per_r == 2) m->h_R.assign(R, R + (size_t)n_r * dim);
    if (m->n_r_pad > 0 && R != nullptr) {
        std::vector<int32_t> r_pad((size_t)m->n_r_pad * dim, 0);
        std::memcpy(r_pad.data(), R, (size_t)n_r * dim * sizeof(int32_t));
        TBK_HIP(hipMalloc(m->d_R.put(), r_pad.size() * sizeof(int32_t)));
        TBK_HIP(hipMemcpy(m->d_R, r_pad.data(), r_pad.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        m->staged_bytes += (int64_t)(r_pad.size() * sizeof(int32_t));
    }
    *out = std::move(guard);
    return TBK_OK;
}

// ------------------------------------------------------------------------------------------------
// model creation / destruction
// ------------------------------------------------------------------------------------------------
extern "C" int tbk_model_create_dense(int device, int dim, int n_orb, int64_t n_r, const int32_t* R,
                                      const double* hop, tbk_model** out) {
    TBK_ARG(out != nullptr, "out is NULL");
    *out = nullptr;
    TBK_ARG(n_r == 0 || hop != nullptr, "hop is NULL");
    ModelGuard guard;
    TBK_CHECK(create_common(device, dim, n_orb, n_r, R, 2, true, &guard));
    tbk_model* m = guard.get();
    m->sparse = false;
    DevPtr<double> d_raw;
    const size_t raw_bytes = (size_t)n_r * n_orb * n_orb * 2 * sizeof(double);
    if (raw_bytes) {
        TBK_HIP(hipMalloc(d_raw.put(), raw_bytes));
        TBK_HIP(hipMemcpyAsync(d_raw, hop, raw_bytes, hipMemcpyHostToDevice, m->stream));
    }
    TBK_CHECK(tbk_stage_dense(m, d_raw));
    TBK_CHECK(tbk_stage_strassen(m));
    TBK_HIP(hipStreamSynchronize(m->stream));
    *out = guard.release();
    return TBK_OK;
}

extern "C" int tbk_model_create_csr(int device, int dim, int n_orb, int64_t n_r, const int32_t* R,
                                    const int64_t* r_ptr, const int32_t* row, const int32_t* col,
                                    const double* val, tbk_model** out) {
    TBK_ARG(out != nullptr, "out is NULL");
    *out = nullptr;
    TBK_ARG(n_r >= 0, "n_r out of range");
    TBK_ARG(n_r == 0 || r_ptr != nullptr, "r_ptr is NULL");
    const int64_t nnz = n_r > 0 ? r_ptr[n_r] : 0;
    TBK_ARG(n_r == 0 || r_ptr[0] == 0, "r_ptr[0] must be 0");
    TBK_ARG(nnz >= 0, "negative nnz");
    TBK_ARG(nnz == 0 || (row && col && val), "row/col/val is NULL");
    for (int64_t r = 0; r < n_r; ++r) TBK_ARG(r_ptr[r] <= r_ptr[r + 1], "r_ptr not monotone");
    for (int64_t t = 0; t < nnz; ++t)
        TBK_ARG(row[t] >= 0 && row[t] < n_orb && col[t] >= 0 && col[t] < n_orb,
                "row/col index out of range");

    ModelGuard guard;
    TBK_CHECK(create_common(device, dim, n_orb, n_r, R, 2, false, &guard));
    tbk_model* m = guard.get();
    m->sparse = true;

    // transpose "per lattice vector, which elements" into "per packed element, which lattice
    // vectors" with a counting sort; record order inside an element follows r (deterministic sums)
    auto packed_index = [n_orb](int i, int j) -> int64_t {  // i <= j
        return (int64_t)i * n_orb - (int64_t)i * (i - 1) / 2 + (j - i);
    };
    std::vector<int64_t> cptr((size_t)m->ncol + 1, 0);
    for (int64_t t = 0; t < nnz; ++t) {
        const int i = std::min(row[t], col[t]), j = std::max(row[t], col[t]);
        cptr[(size_t)packed_index(i, j) + 1]++;
    }
    for (int e = 0; e < m->ncol; ++e) cptr[(size_t)e + 1] += cptr[(size_t)e];
    std::vector<int32_t> rec_r((size_t)nnz);
    std::vector<double> rec_v((size_t)nnz * 2);
    {
        std::vector<int64_t> cursor(cptr.begin(), cptr.end() - 1);
        for (int64_t r = 0; r < n_r; ++r)
            for (int64_t t = r_ptr[r]; t < r_ptr[r + 1]; ++t) {
                const int i = row[t], j = col[t];
                const int kind = (i == j) ? 2 : (i < j ? 0 : 1);
                const int64_t e = packed_index(std::min(i, j), std::max(i, j));
                const int64_t slot = cursor[(size_t)e]++;
                rec_r[(size_t)slot] = (int32_t)((kind << 28) | (int32_t)r);
                rec_v[(size_t)slot * 2] = val[2 * t];
                rec_v[(size_t)slot * 2 + 1] = val[2 * t + 1];
            }
    }
    m->nnz_rec = nnz;
    TBK_HIP(hipMalloc(m->d_cptr.put(), cptr.size() * sizeof(int64_t)));
    TBK_HIP(hipMemcpy(m->d_cptr, cptr.data(), cptr.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    m->staged_bytes += (int64_t)(cptr.size() * sizeof(int64_t));
    if (nnz > 0) {
        TBK_HIP(hipMalloc(m->d_rec_r.put(), (size_t)nnz * sizeof(int32_t)));
        TBK_HIP(hipMalloc(m->d_rec_v.put(), (size_t)nnz * 2 * sizeof(double)));
        TBK_HIP(hipMemcpy(m->d_rec_r, rec_r.data(), (size_t)nnz * sizeof(int32_t), hipMemcpyHostToDevice));
        TBK_HIP(hipMemcpy(m->d_rec_v, rec_v.data(), (size_t)nnz * 2 * sizeof(double), hipMemcpyHostToDevice));
        m->staged_bytes += nnz * (int64_t)(sizeof(int32_t) + 2 * sizeof(double));
        const int kt = tbk_csr_tile_kpoints(n_r);
        if (kt > 0) {
            std::vector<int64_t> sptr;
            std::vector<int32_t> srec_r;
            std::vector<double> srec_v;
            tbk_csr_schedule(m->ncol, kt, cptr, rec_r, rec_v, sptr, srec_r, srec_v);
            m->sched_steps = sptr.back();
            auto upload = [&](auto& dst, const void* src, size_t bytes) -> int {
                TBK_HIP(hipMalloc(dst.put(), std::max<size_t>(bytes, 8)));
                if (bytes) TBK_HIP(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
                m->staged_bytes += (int64_t)bytes;
                return TBK_OK;
            };
            TBK_CHECK(upload(m->d_sptr, sptr.data(), sptr.size() * sizeof(int64_t)));
            TBK_CHECK(upload(m->d_srec_r, srec_r.data(), srec_r.size() * sizeof(int32_t)));
            TBK_CHECK(upload(m->d_srec_v, srec_v.data(), srec_v.size() * sizeof(double)));
            m->sched_kt = kt;
        }
    }
    *out = guard.release();
    return TBK_OK;
}

// The members free themselves (tbk_internal.h: the owning types, destroyed last member first); what is left here is what has to
// hold while they go: the handle's device is current, and nothing is still running on its streams.
extern "C" void tbk_model_destroy(tbk_model* m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    const hipStream_t streams[] = {m->stream, m->stream_eig, m->stream_ql, m->stream_xl[0], m->stream_xl[1], m->stream_xl[2]};
    for (hipStream_t st : streams)
        if (st) (void)hipStreamSynchronize(st);
    delete m;
}

extern "C" int tbk_model_set_option(tbk_model* m, int option, int64_t value) {
    TBK_ARG(m != nullptr, "model is NULL");
    TBK_LOCK(m);
    switch (option) {
        case TBK_OPT_EIGENSOLVER:
            TBK_ARG(value >= TBK_EIG_AUTO && value <= TBK_EIG_ROCSOLVER, "unknown eigensolver");
            m->eigensolver = (int)value;
            return TBK_OK;
        case TBK_OPT_K_CHUNK:
            TBK_ARG(value >= 0, "k chunk must be >= 0");
            m->k_chunk = value;
            return TBK_OK;
        case TBK_OPT_TIMING:
            m->timing = value != 0;
            return TBK_OK;
        case TBK_OPT_FOLD:
            m->fold_enabled = value != 0;
            return TBK_OK;
        case TBK_OPT_STRASSEN:
            m->strassen = value != 0;
            return TBK_OK;
        case TBK_OPT_STRASSEN_LEVELS:
            TBK_ARG(value == 1 || value == 2, "Strassen levels must be 1 or 2");
            m->strassen_levels = (int)value;
            return TBK_OK;
        case TBK_OPT_STRASSEN_COMBINE:
            TBK_ARG(value == 0 || value == 1, "the Strassen combine is 0 (one kernel) or 1 (two passes)");
            m->strassen_combine_split = value != 0;
            return TBK_OK;
        default:
            tbk_set_error("unknown option %d", option);
            return TBK_ERR_ARGUMENT;
    }
}

extern "C" int tbk_model_info(const tbk_model* m, int* device, int* dim, int* n_orb, int64_t* n_r,
                              int* is_sparse, int64_t* staged_bytes) {
    TBK_ARG(m != nullptr, "model is NULL");
    if (device) *device = m->device;
    if (dim) *dim = m->dim;
    if (n_orb) *n_orb = m->n_orb;
    if (n_r) *n_r = m->n_r;
    if (is_sparse) *is_sparse = m->sparse ? 1 : 0;
    if (staged_bytes) *staged_bytes = m->staged_bytes;
    return TBK_OK;
}

// ------------------------------------------------------------------------------------------------
// the chunked pipeline
// ------------------------------------------------------------------------------------------------
int64_t choose_chunk(tbk_model* m, int64_t nk, bool with_eig) {
    // (a call of up to one k tile is one chunk whatever the memory: no hipMemGetInfo -- a driver query -- on the one-k path)
    if (nk <= TBK_BM) return TBK_BM;
    const int64_t n = m->n_orb;
    int64_t per_k = m->k2 * 8 + (with_eig ? n * n * 16 + (int64_t)tbk_eig_scratch_per_k(m) : 0);
    if (per_k < 64) per_k = 64;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = size_t(8) << 30;
    // (what this handle's grow-only chunk workspaces hold already is as good as free: counted out, the second call of a model
    // chose a smaller chunk than the first -- cfg3: one chunk in the warm-up, two from then on)
    free_b += m->ws_H.bytes + m->ws_H2.bytes + m->ws_phase.bytes + m->ws_band.bytes + m->ws_bandmat[0].bytes + m->ws_bandmat[1].bytes +
              m->ws_E.bytes + m->ws_xl.bytes + m->ws_part.bytes + m->ws_c11.bytes;
    // above 64 orbitals a chunk is a few thousand matrices: every kernel of the eigensolver ends on a partly filled
    // round of workgroups, and 2 - 3 times longer chunks were worth 3 - 4 % (cfg3 3846 -> 12500 matrices per chunk,
    // cfg5 1250 -> 5000)
    // Round 6: 65 - 256 orbitals take chunks as long as 64 GiB allow (up to 131072 k-points).  At these sizes the reduction is
    // ~90 % of a chunk and its neighbours in the pipeline (the next chunk's H(k), the previous chunk's bisection) run on the
    // same FP64 pipes: overlapping them buys nothing, every chunk boundary costs the partly filled last rounds of its kernels
    // -- whole eigenval, us per k-point, chunks of 16384 / 32768 / 65536 / 131072: 0.4095 / 0.4060 / 0.4041 / 0.4024 at 96
    // orbitals, 2.291 / 2.264 / 2.247 / 2.228 at 160, 5.668 / 5.586 / 5.531 / 5.518 at 256; cfg3 170.8 -> 176.4 k k-points/s in ONE
    // chunk.  Above 256 orbitals the second stage is a launch of its own that does fill gaps: cfg5 16.63 k in chunks of 4096,
    // 16.51 k in one.
    const bool mid = n > 64 && n <= 256;
    int64_t budget = std::min<int64_t>((int64_t)(free_b / 4), int64_t(mid ? 64 : n > 64 ? 24 : 6) << 30);
    int64_t chunk = budget / per_k / TBK_BM * TBK_BM;
    // 32768 k-points per chunk at 64 orbitals and above; small matrices take proportionally more (up to 1 M at 8
    // orbitals): a chunk is ~6 launches and one QL latency chain whatever its size, and 20 M k-points of an
    // 8-orbital model spent 42 of 92 GPU-ms in 612 of those chains
    int64_t cap = mid ? 131072 : 32768;
    if (n < 64) cap *= std::min<int64_t>(32, (64 / n) * (64 / n));
    chunk = std::max<int64_t>(TBK_BM, std::min<int64_t>(chunk, cap));
    tbk_hk_plan_t plan = tbk_hk_plan(m, tbk_staged_operand(m), std::min(chunk, nk), false);
    if (plan.path == HK_PATH_STRASSEN2) {
        // The first two-level chunk of a model builds the operand blocks of the second level (fill_rows): decided here, where
        // the memory is counted -- blocks above a quarter of the free memory are skipped, and the model stays on one level.
        // Such a chunk holds its phase rows 49/16 times (As2[49][K2 / 4][Mq]) and the 49 quarter-size products
        // P[49][Mq][ncol_pad / 4], and with the two-pass combine of the eigenvalue path the four partial C11 quarters
        // [4][Mq][ncol_pad / 4] between the passes; a chunk that does not fit gets shorter, and below TBK_STRASSEN2_MIN_NK it takes one level
        size_t free2 = free_b;
        if (m->d_Bs2 == nullptr) {
            const size_t blocks = tbk_strassen2_bytes(m);
            if (blocks > free_b / 4) m->bs2_skipped = true;
            else free2 -= blocks;
        }
        if (!m->bs2_skipped) {
            const int64_t per_k_s = per_k + m->k2 * 8 * 33 / 16 + (int64_t)m->ncol_pad * 16 * 49 / 16 + (with_eig && m->strassen_combine_split ? (int64_t)m->ncol_pad * 16 * 4 / 16 : 0);
            const int64_t fit = (int64_t)(free2 / 4) / per_k_s / TBK_BM * TBK_BM;
            chunk = std::max<int64_t>(TBK_BM, std::min(chunk, fit));
        }
        plan = tbk_hk_plan(m, tbk_staged_operand(m), std::min(chunk, nk), false);
    }
    if (plan.path == HK_PATH_STRASSEN) {
        // a Strassen chunk also holds its phase rows 7/4 times (As[7][K2 / 2][Mh]) and the seven half-size products
        // P[7][Mh][ncol_pad / 2] (re, im): that must fit the quarter of the free memory -- else a shorter chunk (classical
        // below TBK_STRASSEN_MIN_NK k-points)
        const int64_t per_k_s = per_k + m->k2 * 8 * 3 / 4 + (int64_t)m->ncol_pad * 16 * 7 / 4;
        const int64_t fit = (int64_t)(free_b / 4) / per_k_s / TBK_BM * TBK_BM;
        chunk = std::max<int64_t>(TBK_BM, std::min(chunk, fit));
    }
    if (m->k_chunk > 0) chunk = round_up(m->k_chunk, TBK_BM);
    else if (chunk >= 4096) chunk = chunk / 4096 * 4096;  // 32 k tiles: equal shares for the 8 XCDs
    return std::min(chunk, round_up(nk, TBK_BM));
}

// The phase rows of a chunk of plan.nk k-points for its plan (the lattice of plan.op), in ws_phase (reserved also when the H(k) kernel makes them).
int fill_rows(tbk_model* m, const tbk_hk_plan_t& plan, const double* d_k) {
    TBK_CHECK(m->ws_phase.reserve((size_t)plan.row_doubles * sizeof(double)));
    double* d_A = m->ws_phase.as<double>();
    if (plan.rows == HK_ROWS_NONE) return TBK_OK;
    if (plan.rows == HK_ROWS_STRASSEN) return tbk_launch_phase_strassen(m, plan.op, d_k, plan.nk, d_A);  // the seven blocks of its left operands
    if (plan.rows == HK_ROWS_STRASSEN2) {
        TBK_CHECK(tbk_stage_strassen2(m));  // the right operands of the second level, on the model's first two-level chunk
        return tbk_launch_phase_strassen2(m, plan.op, d_k, plan.nk, d_A);  // the 49 blocks of its left operands
    }
    if (plan.rows == HK_ROWS_MONOMIAL)
        return tbk_launch_monomials(m->stream, m->d_powers, plan.op.dim, plan.op.n_r, plan.op.k2, d_k, plan.nk, plan.nk_pad, d_A);
    return tbk_launch_phase(m, plan.op, d_k, plan.nk, plan.nk_pad, d_A);
}

// H(k) of the chunk whose rows fill_rows made for the same plan: the second half of chunk_h
static int build_h(tbk_model* m, const tbk_hk_plan_t& plan, int mode, int convention, const double* d_k, const double* d_pos_raw,
                   const tbk_one_k_t& one_k, double* d_H) {
    const double* d_A = plan.rows == HK_ROWS_NONE ? nullptr : m->ws_phase.as<double>();
    const double* d_orb = nullptr;
    // (a one-k host call: the H(k) kernel forms the phases of its one k-point itself from one_k's raw positions)
    if (convention == 1 && one_k.h_k == nullptr) {
        TBK_CHECK(m->ws_orb.reserve((size_t)plan.nk * m->n_orb * 2 * sizeof(double)));
        TBK_CHECK(tbk_launch_orbital_phases(m, d_k, d_pos_raw, plan.nk, m->ws_orb.as<double>()));
        d_orb = m->ws_orb.as<double>();
    }
    TBK_ARG(plan.path != HK_PATH_CSR || one_k.h_k == nullptr, "sparse models read k from the device");
    if (plan.path == HK_PATH_CSR) return tbk_launch_hk_csr(m, d_A, plan.nk, plan.nk_pad, mode, convention, d_k, d_orb, d_H);
    return tbk_launch_hk_dense(m, plan, d_A, mode, convention, d_k, d_orb, one_k, d_H);
}

int chunk_h(tbk_model* m, const tbk_hk_plan_t& plan, int mode, int convention, const double* d_k, const double* d_pos_raw,
            const tbk_one_k_t& one_k, double* d_H) {
    TBK_CHECK(fill_rows(m, plan, d_k));
    return build_h(m, plan, mode, convention, d_k, d_pos_raw, one_k, d_H);
}

int tbk_chunk_dh(tbk_model* m, int axis, const double* d_k, int64_t nk, double* d_D) {
    const int64_t chunk = choose_chunk(m, nk, false);
    const size_t nn2 = (size_t)m->n_orb * m->n_orb * 2;
    for (int64_t c0 = 0; c0 < nk; c0 += chunk) {
        const int64_t nkc = std::min(chunk, nk - c0);
        const tbk_hk_plan_t plan = tbk_hk_plan(m, tbk_staged_operand(m), nkc, true, true);
        TBK_CHECK(m->ws_phase.reserve((size_t)plan.row_doubles * sizeof(double)));
        TBK_CHECK(tbk_launch_phase_derivative(m, plan.op, d_k + c0 * m->dim, nkc, plan.nk_pad, axis, m->ws_phase.as<double>()));
        TBK_CHECK(build_h(m, plan, HK_FULL, 2, d_k + c0 * m->dim, nullptr, tbk_one_k_t(), d_D + (size_t)c0 * nn2));
    }
    return TBK_OK;
}

extern "C" int tbk_hamilton_derivative_device(tbk_model* m, const double* d_k, int64_t nk, int axis, double* d_D) {
    TBK_ARG(m != nullptr, "model is NULL");
    TBK_LOCK(m);
    TBK_ARG(!m->kdotp, "k.p models have no lattice vectors to differentiate");
    TBK_ARG(axis >= 0 && axis < m->dim, "axis must be 0 ... dim - 1");
    TBK_ARG(nk >= 0, "nk < 0");
    if (nk == 0) return TBK_OK;
    TBK_ARG(d_k && d_D, "k / D is NULL");
    TBK_HIP(hipSetDevice(m->device));
    return tbk_chunk_dh(m, axis, d_k, nk, d_D);
}

// FULL H(k) of nk k-points on the device, chunk by chunk (the caller holds the lock and has checked the arguments)
static int hamilton_chunks(tbk_model* m, const double* d_k, int64_t nk, int convention, const double* d_pos, const tbk_one_k_t& one_k, double* d_H) {
    const int64_t chunk = choose_chunk(m, nk, false);
    const size_t nn2 = (size_t)m->n_orb * m->n_orb * 2;
    for (int64_t c0 = 0; c0 < nk; c0 += chunk) {
        const int64_t nkc = std::min(chunk, nk - c0);
        const tbk_hk_plan_t plan = tbk_hk_plan(m, tbk_staged_operand(m), nkc, false);
        TBK_CHECK(chunk_h(m, plan, HK_FULL, convention, d_k + c0 * m->dim, d_pos, one_k, d_H + (size_t)c0 * nn2));
    }
    return TBK_OK;
}

extern "C" int tbk_hamilton_device(tbk_model* m, const double* d_k, int64_t nk, int convention,
                                   const double* d_pos, double* d_H) {
    TBK_ARG(m != nullptr, "model is NULL");
    TBK_LOCK(m);
    TBK_ARG(convention == 1 || convention == 2, "convention must be 1 or 2");
    TBK_ARG(nk >= 0, "nk < 0");
    if (nk == 0) return TBK_OK;
    TBK_ARG(d_k && d_H, "k / H is NULL");
    TBK_ARG(convention == 2 || d_pos != nullptr, "convention 1 needs pos");
    TBK_HIP(hipSetDevice(m->device));
    return hamilton_chunks(m, d_k, nk, convention, d_pos, tbk_one_k_t(), d_H);
}

// Eigenvalues with the hand-written solvers (the reduction family of the call's tbk_eig_plan), software-pipelined over k
// chunks on three streams:   main: phase(c) -> H(c)      eig: tridiag(c)      ql: QL(c - 1)
//
//     | H(c) | tridiag(c) || QL(c-1) | H(c+1) | tridiag(c+1) || QL(c) | ...
//
// The MFMA contraction runs alone: it fills the LDS (2 x 72 KiB per CU), so anything co-scheduled with
// it only displaces its workgroups.  The two eigensolver kernels are complementary -- the reduction is
// VALU-bound with 14 KiB of LDS per workgroup, the QL is a latency-bound serial chain with 64 KiB per
// workgroup and almost no issue pressure -- so QL(c-1) runs in the shadow of tridiag(c).
// tridiagonal stage on the QL stream: lane-per-matrix QL or bisection, as the plan says.  Per launch, not in the plan:
// `beside_ql` (tbk_launch_ql), `bisect_anyway` (the last chunk of a pipeline has no reduction to hide a QL chain behind), and
// d_band (the second stage of this chunk runs here first)
static int launch_tridiag_eigenvalues(tbk_model* m, const tbk_eig_plan_t& plan, hipStream_t s, double* d_de, int64_t nk, double* d_E,
                                      bool beside_ql = false, bool bisect_anyway = false, const void* d_band = nullptr) {
    // two-stage reduction: the second stage (band -> tridiagonal) of this chunk runs here, in front of its bisection --
    // on the tridiagonal stream, i.e. next to the first stage of the following chunk
    if (d_band) TBK_CHECK(tbk_launch_band_chase(m, plan, s, d_band, nk, d_de));
    if (!plan.bisect && !bisect_anyway) return tbk_launch_ql(m, s, d_de, nk, d_E, beside_ql);
    return tbk_launch_bisect(m, plan, s, d_de, nk, d_E);
}

// k chunks of the pipeline.  The lane-per-matrix QL is a latency chain (~3 ms however few matrices it
// gets), and the QL of the last chunk has nothing to hide behind: the schedule therefore ends on a short
// chunk (one XCD round of k tiles plus the ragged remainder) whose reduction is brief, and that chunk's QL
// runs next to the QL of the chunk before it.  All other chunks are multiples of 4096 k-points.
//
// The short chunk is one unit longer (two units plus the remainder) where that moves it from a slower contraction path onto
// two Strassen levels: tbk_hk_plan is asked for both lengths, its thresholds are not repeated here.  Models whose chunks never
// take two levels, and the folded builder (`direct` false), keep one unit plus the remainder.  Measured at the headline shape
// (64 orbitals, 4096 lattice vectors, 100 000 k-points; tools/sweep_strassen.py, contraction + rows of one chunk, ms):
//     one level, 5792 k-points     5.219 + 0.110        two levels, 28672    21.264 + 1.085
//     two levels, 9888             7.591 + 0.324        two levels, 32768    24.194 + 1.263
// 32768 + 32768 + 28672 + 5792 is 78.59 ms, 32768 + 28672 + 28672 + 9888 is 78.07: the last chunk pays 2.59 ms for the
// 4096 k-points that cost a long chunk 3.11 (0.76 us per k-point).  The reduction and bisection of the longer last chunk
// are exposed as before; only the bisection's share grows (~0.05 ms).  `python bench.py`, old and new rule alternating, five
// runs each: 86.49 -> 85.72 ms per step (medians; 86.43 - 86.89 and 85.29 - 85.76).
static std::vector<int64_t> chunk_schedule(tbk_model* m, int64_t nk, int64_t chunk, bool direct) {
    std::vector<int64_t> out;
    const int64_t unit = 4096;
    if (!tbk_eig_small_supported(m->n_orb) || m->k_chunk > 0 || chunk < 2 * unit || nk < 3 * unit) {
        for (int64_t c0 = 0; c0 < nk; c0 += chunk) out.push_back(std::min(chunk, nk - c0));
        return out;
    }
    int64_t last = unit + nk % unit;  // in [4096, 8192)
    if (direct && last + unit <= chunk) {
        const tbk_operand_t op = tbk_staged_operand(m);
        const HkPath shorter = tbk_hk_plan(m, op, last, false).path;
        if (tbk_hk_plan(m, op, last + unit, false).path == HK_PATH_STRASSEN2 && (shorter == HK_PATH_STRASSEN || shorter == HK_PATH_TILES))
            last += unit;  // in [8192, 12288)
    }
    int64_t rest = nk - last;  // a multiple of 4096
    const int64_t n_big = (rest + chunk - 1) / chunk;
    for (int64_t i = 0; i < n_big; ++i) {
        // as even as whole units allow, larger chunks first
        const int64_t share = round_up((rest + (n_big - i) - 1) / (n_big - i), unit);
        const int64_t take = std::min(std::min(share, chunk), rest);
        out.push_back(take);
        rest -= take;
    }
    out.push_back(last);
    return out;
}

// Fills H for k-points [c0, c0 + nkc) of the call (phase rows + contraction on the main stream).
using HBuilder = std::function<int(int64_t c0, int64_t nkc, double* d_H)>;

// one_k: for the direct builder (a folded call never is a one-k call).  on_chunk (NULL: none): tbk_chunk_hook_t, tbk_internal.h.
static int eigenval_wave_pipeline(tbk_model* m, const tbk_eig_plan_t& plan, const double* d_k, int64_t nk, double* d_E,
                                  const tbk_one_k_t& one_k, const tbk_chunk_hook_t* on_chunk, const HBuilder* builder = nullptr,
                                  const std::vector<int64_t>* runs = nullptr) {
    // The direct builder in two halves: the phase rows of a chunk only need the previous contraction to be done with the
    // row buffer (stream order), not the eigensolver to be done with H -- so they are enqueued BEFORE the main stream
    // waits for the previous chunk's reduction and run under it (an HBM-write kernel beside a VALU-bound one: 1.5 ms
    // per 100 k k-points at the headline shape).
    int64_t rows_ready_for = -1;  // c0 of the chunk whose phase rows are in ws_phase, made for rows_plan
    tbk_hk_plan_t rows_plan;
    const auto prepare_rows = [&](int64_t c0, int64_t nkc) -> int {
        rows_plan = tbk_hk_plan(m, tbk_staged_operand(m), nkc, false);
        if (rows_plan.rows != HK_ROWS_NONE) TBK_CHECK(fill_rows(m, rows_plan, d_k + c0 * m->dim));
        rows_ready_for = c0;
        return TBK_OK;
    };
    const HBuilder direct = [&](int64_t c0, int64_t nkc, double* d_H) -> int {
        if (rows_ready_for != c0) TBK_CHECK(prepare_rows(c0, nkc));
        return build_h(m, rows_plan, HK_TRI, 2, d_k + c0 * m->dim, nullptr, one_k, d_H);
    };
    const HBuilder& build = builder ? *builder : direct;
    const int64_t chunk = choose_chunk(m, nk, true);
    const size_t n = (size_t)m->n_orb;
    const size_t nn2 = n * n * 2;
    DevBuf* debuf[2] = {&m->ws_E, &m->ws_E2};
    const std::vector<int64_t> sched =
        (runs != nullptr && m->k_chunk == 0 && nk > chunk) ? run_schedule(*runs, chunk) : chunk_schedule(m, nk, chunk, builder == nullptr);
    const int64_t n_chunks = (int64_t)sched.size();
    const int64_t max_chunk = *std::max_element(sched.begin(), sched.end());
    TBK_CHECK(m->ws_H.reserve((size_t)max_chunk * nn2 * sizeof(double)));
    for (int b = 0; b < (n_chunks > 1 ? 2 : 1); ++b)
        TBK_CHECK(debuf[b]->reserve((size_t)max_chunk * n * 2 * sizeof(double)));
    double* d_H = m->ws_H.as<double>();
    // Folded H(k) (a mesh: ~30 small launches per chunk, 1.05 of the 5.5 ms a 32768-point chunk of cfg4 takes) is
    // built BESIDE the reduction of the previous chunk, into a second H buffer; chunk c then waits for the reduction
    // of chunk c - 2.  (Not for the direct contraction, which fills the chip and shares the FP64 pipe: see above.)
    // Round 4, MEASURED AND LEFT OFF (DESIGN_LOG.md R4.15): the same for the direct H(k) of the two-stage sizes (from 185
    // orbitals) -- that reduction is a chain of short phases which leaves the matrix pipe idle four fifths of the time, and
    // the sparse H(k) is an HBM-write kernel.  There: one after the other (the round-3 order).
    const bool h_overlap = n_chunks > 2 && builder != nullptr && plan.family == EIG_REGISTER;
    double* d_Hbuf[2] = {d_H, d_H};
    if (h_overlap) {
        TBK_CHECK(m->ws_H2.reserve((size_t)max_chunk * nn2 * sizeof(double)));
        d_Hbuf[1] = m->ws_H2.as<double>();
    }
    // two-stage reduction in two launches (above 256 orbitals): stage two of a chunk goes to the tridiagonal stream; fused
    // (up to 256) it is part of the reduction kernel and this flag stays off.  (Of the launch, not of the plan: one chunk has
    // no following chunk to run beside.)
    const bool two_stage = plan.family == EIG_TWO_STAGE && !plan.fused && n_chunks > 1;
    TBK_CHECK(tbk_eig_reserve(m, plan, max_chunk, n_chunks > 1 ? 2 : 1));
    if (n_chunks == 1) {
        // one chunk has nothing to overlap: everything in order on the main stream, and the pipeline adds no cross-stream
        // events (they cost more than the kernels of a single-k call).  A chunk long enough for two Strassen levels (from
        // TBK_STRASSEN2_MIN_NK k-points, ~7 ms of products) does cross to stream_eig and back inside launch_strassen2, for the
        // first pass of its combine; H is complete on the main stream when build() returns either way.
        double* d_de = debuf[0]->as<double>();
        TBK_CHECK(build(0, nk, d_H));
        TBK_CHECK(tbk_eig_reduce(m, plan, m->stream, d_H, nk, d_de));
        TBK_CHECK(launch_tridiag_eigenvalues(m, plan, m->stream, d_de, nk, d_E));
        if (on_chunk) {
            TBK_HIP(hipEventRecord(m->ev_ql[0], m->stream));
            TBK_CHECK((*on_chunk)(0, nk, m->ev_ql[0]));
        }
        return TBK_OK;
    }
    int64_t prev_c0 = 0, prev_nkc = 0, c0 = 0;
    for (int64_t c = 0; c < n_chunks; ++c) {
        const int b = (int)(c & 1);
        const int64_t nkc = sched[c];
        double* d_de = debuf[b]->as<double>();
        d_H = d_Hbuf[b];
        if (c >= 1) {
            if (!builder) TBK_CHECK(prepare_rows(c0, nkc));  // under the previous chunk's reduction
            // H(c) overwrites an H buffer; the direct contraction must not share the chip with the eigensolver either
            if (!h_overlap)
                TBK_HIP(hipStreamWaitEvent(m->stream, m->ev_tri[b ^ 1], 0));
            else if (c >= 2)
                TBK_HIP(hipStreamWaitEvent(m->stream, m->ev_tri[b], 0));
            // (d, e) of chunk c - 2 must have been consumed before the reduction of chunk c overwrites them; beside
            // the previous reduction, H(c) itself need not wait for that
            if (c >= 2 && !h_overlap) TBK_HIP(hipStreamWaitEvent(m->stream, m->ev_ql[b], 0));
        }
        TBK_CHECK(build(c0, nkc, d_H));
        TBK_HIP(hipEventRecord(m->ev_hk[b], m->stream));

        TBK_HIP(hipStreamWaitEvent(m->stream_eig, m->ev_hk[b], 0));
        if (c >= 2 && h_overlap) TBK_HIP(hipStreamWaitEvent(m->stream_eig, m->ev_ql[b], 0));
        TBK_CHECK(tbk_eig_reduce(m, plan, m->stream_eig, d_H, nkc, d_de, two_stage ? m->ws_bandmat[b].ptr : nullptr));
        TBK_HIP(hipEventRecord(m->ev_tri[b], m->stream_eig));

        if (c >= 1) {  // tridiagonal stage of the previous chunk, alongside this chunk's reduction
            TBK_HIP(hipStreamWaitEvent(m->stream_ql, m->ev_hk[b], 0));
            // (d, e) of the previous chunk: implied by ev_hk unless H(c) was built beside that reduction
            if (h_overlap) TBK_HIP(hipStreamWaitEvent(m->stream_ql, m->ev_tri[b ^ 1], 0));
            TBK_CHECK(launch_tridiag_eigenvalues(m, plan, m->stream_ql, debuf[b ^ 1]->as<double>(), prev_nkc,
                                                 d_E + (size_t)prev_c0 * n, false, false,
                                                 two_stage ? m->ws_bandmat[b ^ 1].ptr : nullptr));
            TBK_HIP(hipEventRecord(m->ev_ql[b ^ 1], m->stream_ql));
            if (on_chunk) TBK_CHECK((*on_chunk)(prev_c0, prev_nkc, m->ev_ql[b ^ 1]));
        }
        prev_c0 = c0;
        prev_nkc = nkc;
        c0 += nkc;
    }
    {  // Eigenvalues of the last chunk, behind its own reduction on the eig stream, i.e. next to QL(last - 1).
       // Nothing is left to hide a 2.7 ms QL chain behind: the (short) last chunk takes the bisection kernel,
       // a wave per matrix for ~0.1 ms (measured: 2.6 ms off the 100k step).
        const int b = (int)((n_chunks - 1) & 1);
        TBK_CHECK(launch_tridiag_eigenvalues(m, plan, m->stream_eig, debuf[b]->as<double>(), prev_nkc,
                                             d_E + (size_t)prev_c0 * n, true, true, two_stage ? m->ws_bandmat[b].ptr : nullptr));
        TBK_HIP(hipEventRecord(m->ev_ql[b], m->stream_eig));
        if (on_chunk) TBK_CHECK((*on_chunk)(prev_c0, prev_nkc, m->ev_ql[b]));
    }
    // later work on the main stream (gather, D2H, the next call) sees the finished eigenvalues
    for (int b = 0; b < (n_chunks > 1 ? 2 : 1); ++b) TBK_HIP(hipStreamWaitEvent(m->stream, m->ev_ql[b], 0));
    TBK_HIP(hipStreamWaitEvent(m->stream, m->ev_tri[(n_chunks - 1) & 1], 0));
    return TBK_OK;
}

// k lists with long runs of one shared component (grids in meshgrid order, stacks of planes): the pipeline above with the
// H(k) builder of tbk_folded_call (tbk_fold.hip).  A list that does not qualify, and every one-k call, takes the direct builder.
static int eigenval_folded(tbk_model* m, const tbk_eig_plan_t& eig_plan, const double* d_k, const double* h_k, int64_t nk, double* d_E,
                           const tbk_one_k_t& one_k, const tbk_chunk_hook_t* on_chunk) {
    tbk_folded_call call(m, d_k, h_k, nk);
    if (one_k.h_k != nullptr || !call.folds()) return eigenval_wave_pipeline(m, eig_plan, d_k, nk, d_E, one_k, on_chunk);
    TBK_CHECK(call.begin());
    const HBuilder folded = [&call](int64_t c0, int64_t nkc, double* d_H) { return call.build(c0, nkc, d_H); };
    TBK_CHECK(eigenval_wave_pipeline(m, eig_plan, d_k, nk, d_E, one_k, on_chunk, &folded, &call.runs));
    m->counters[TBK_CNT_FOLDED_CALLS] += 1;
    m->counters[TBK_CNT_FOLDED_KPOINTS] += nk;
    return TBK_OK;
}

// NaN / Inf anywhere in the hoppings or in k reaches the eigenvalues (the solvers write NaN for a non-finite matrix):
// scipy's eigvalsh(check_finite=True) raises there (_tb_model.py:1147-1150).  One pass over the finished eigenvalues
// on the device raises the flag that tbk_eigenval_check turns into TBK_ERR_NOT_FINITE -- the host-side
// np.isfinite(out).all() it replaces cost 80 ms for 20 M k-points of an 8-orbital model, as much as all the kernels.
__global__ void __launch_bounds__(256) flag_nonfinite_kernel(const double* __restrict__ E, int64_t total, int* __restrict__ flag) {
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) bad |= !isfinite(E[i]);
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicAdd(flag, 1);
}

// plan: tbk_eig_plan of this call, made once by the entry point (which holds the lock); everything below reads it.  h_k: the
// caller's host copy of the list for the fold analysis, or NULL; one_k: set by tbk_eigenval alone.
static int eigenval_device_impl(tbk_model* m, const tbk_eig_plan_t& plan, const double* d_k, const double* h_k, int64_t nk, double* d_E,
                                const tbk_one_k_t& one_k, const tbk_chunk_hook_t* on_chunk) {
    TBK_ARG(nk >= 0, "nk < 0");
    if (nk == 0) return TBK_OK;
    TBK_ARG(d_k && d_E, "k / E is NULL");
    TBK_HIP(hipSetDevice(m->device));
    m->counters[TBK_CNT_EIGENVAL_CALLS] += 1;
    TBK_CHECK(tbk_eig_check_option(m));
    // the library's own reduction kernels (the chunk pipeline), not rocSOLVER.  They raise the flag themselves (QL and
    // bisection see every non-finite (d, e) and answer NaN); rocSOLVER's eigenvalues get the pass over the output
    if (plan.own()) return eigenval_folded(m, plan, d_k, h_k, nk, d_E, one_k, on_chunk);
    TBK_ARG(one_k.h_k == nullptr, "the rocSOLVER branch fills its phase rows from k on the device");

    int64_t chunk = choose_chunk(m, nk, true);
    const size_t nn2 = (size_t)m->n_orb * m->n_orb * 2;
    // rocsolver_zheevd_strided_batched faulted (memory access fault inside the library) on 2048 matrices of 768 / 1024
    // orbitals -- 1.2e9 / 2.1e9 complex elements in one call -- and ran 2048 x 640 (8.4e8): calls are kept below 2^29
    // elements
    chunk = std::max<int64_t>(1, std::min<int64_t>(chunk, (int64_t(1) << 29) / std::max<int64_t>(1, (int64_t)m->n_orb * m->n_orb)));
    // rocSOLVER path: TBK_EIG_ROCSOLVER, or n_orb above the own solvers' range
    m->counters[TBK_CNT_LIBRARY_CALLS] += 1;
    for (int64_t c0 = 0; c0 < nk; c0 += chunk) {
        const int64_t nkc = std::min(chunk, nk - c0);
        const tbk_hk_plan_t hk = tbk_hk_plan(m, tbk_staged_operand(m), nkc, true);
        TBK_CHECK(m->ws_H.reserve((size_t)nkc * nn2 * sizeof(double)));
        double* d_H = m->ws_H.as<double>();
        TBK_CHECK(chunk_h(m, hk, HK_TRI, 2, d_k + c0 * m->dim, nullptr, tbk_one_k_t(), d_H));
        TBK_CHECK(tbk_eig_batched(m, d_H, nkc, d_E + (size_t)c0 * m->n_orb));
    }
    {
        const int64_t total = nk * m->n_orb;
        const unsigned blocks = (unsigned)std::min<int64_t>((total + 255) / 256, 8 * 1024);
        hipLaunchKernelGGL(flag_nonfinite_kernel, dim3(blocks), dim3(256), 0, m->stream, d_E, total, m->ws_flag.as<int>() + 1);
        TBK_HIP(hipGetLastError());
    }
    return TBK_OK;
}

int tbk_eigenval_device_hooked(tbk_model* m, const double* d_k, const double* h_k, int64_t nk, double* d_E, const tbk_chunk_hook_t* on_chunk) {
    TBK_ARG(m != nullptr, "model is NULL");
    TBK_LOCK(m);
    return eigenval_device_impl(m, tbk_eig_plan(m->n_orb, m->eigensolver, nk), d_k, h_k, nk, d_E, tbk_one_k_t(), on_chunk);
}

extern "C" int tbk_eigenval_device_hint(tbk_model* m, const double* d_k, const double* h_k, int64_t nk, double* d_E) {
    return tbk_eigenval_device_hooked(m, d_k, h_k, nk, d_E, nullptr);
}

extern "C" int tbk_eigenval_device(tbk_model* m, const double* d_k, int64_t nk, double* d_E) {
    return tbk_eigenval_device_hint(m, d_k, nullptr, nk, d_E);
}

extern "C" int tbk_eigenval_schedule(tbk_model* m, int64_t nk, int64_t* lengths, int capacity, int* n_chunks) {
    TBK_ARG(m != nullptr && n_chunks != nullptr, "model / n_chunks is NULL");
    TBK_ARG(nk >= 1, "nk < 1");
    TBK_ARG(capacity >= 0 && (lengths != nullptr || capacity == 0), "lengths is NULL");
    TBK_LOCK(m);
    TBK_ARG(tbk_eig_plan(m->n_orb, m->eigensolver, nk).own(), "the eigenvalue calls of this model go to rocSOLVER, not through the chunk pipeline");
    TBK_HIP(hipSetDevice(m->device));
    const std::vector<int64_t> sched = chunk_schedule(m, nk, choose_chunk(m, nk, true), true);
    *n_chunks = (int)sched.size();
    for (size_t i = 0; i < sched.size() && (int)i < capacity; ++i) lengths[i] = sched[i];
    return TBK_OK;
}

extern "C" int tbk_model_counter(tbk_model* m, int counter, int64_t* value) {
    TBK_ARG(m != nullptr && value != nullptr, "model / value is NULL");
    TBK_ARG(counter >= 0 && counter < TBK_CNT_COUNT, "unknown counter");
    TBK_LOCK(m);
    *value = m->counters[counter];
    return TBK_OK;
}

// Wait for everything enqueued on the main stream -- through an event.  hipStreamSynchronize on this runtime goes to sleep
// for ~250 us in calls whose GPU work takes a few tens of microseconds (one-k hamilton / eigenval: 290 instead of 50 - 90 us
// per call, tools/trace_single_k.py); hipEventSynchronize on an event recorded at the same point does not.
static int wait_main_stream(tbk_model* m) {
    TBK_HIP(hipEventRecord(m->ev_sync, m->stream));
    TBK_HIP(hipEventSynchronize(m->ev_sync));
    return TBK_OK;
}

extern "C" int tbk_synchronize(tbk_model* m) {
    TBK_ARG(m != nullptr, "model is NULL");
    TBK_LOCK(m);
    TBK_HIP(hipSetDevice(m->device));
    return wait_main_stream(m);
}

extern "C" int tbk_eigenval_check(tbk_model* m) {
    TBK_ARG(m != nullptr, "model is NULL");
    TBK_LOCK(m);
    TBK_HIP(hipSetDevice(m->device));
    int flag[2] = {0, 0};
    TBK_HIP(hipMemcpyAsync(flag, m->ws_flag.ptr, sizeof(flag), hipMemcpyDeviceToHost, m->stream));
    TBK_HIP(hipMemsetAsync(m->ws_flag.ptr, 0, sizeof(flag), m->stream));
    TBK_CHECK(wait_main_stream(m));
    if (flag[1] != 0) {
        tbk_set_error("array must not contain infs or NaNs");  // scipy's message for the same condition
        return TBK_ERR_NOT_FINITE;
    }
    if (flag[0] != 0) {
        tbk_set_error("eigensolver did not converge for %d matrices", flag[0]);
        return TBK_ERR_NO_CONVERGENCE;
    }
    return TBK_OK;
}

// ---- host-buffer entry points -------------------------------------------------------------------
// H leaves the device in chunks through two buffers, chunk c + 1 being computed while chunk c crosses PCIe: 20 000
// k-points at N_orb = 64, N_R = 4096 in 25 ms instead of 46 (52 GB/s) when the caller's array has been written before.
// A FRESH result array (np.empty: no pages behind it yet) is bound by the kernel's page-fault rate instead, ~21 GB/s
// on these hosts whoever takes the faults: populating the pages from helper threads (MADV_HUGEPAGE +
// MADV_POPULATE_WRITE, four threads, ahead of the copy or racing it) did not beat the copy thread faulting by itself
// (66 vs 57 ms for 1.3 GB), so there is no such helper here.
extern "C" int tbk_hamilton(tbk_model* m, const double* k, int64_t nk, int convention,
                            const double* pos, double* H_out) {
    TBK_ARG(m != nullptr, "model is NULL");
    TBK_LOCK(m);
    TBK_ARG(convention == 1 || convention == 2, "convention must be 1 or 2");
    TBK_ARG(nk >= 0, "nk < 0");
    if (nk == 0) return TBK_OK;
    TBK_ARG(k && H_out, "k / H is NULL");
    TBK_ARG(convention == 2 || pos != nullptr, "convention 1 needs pos");
    TBK_HIP(hipSetDevice(m->device));
    const size_t nn2 = (size_t)m->n_orb * m->n_orb * 2;
    {
        const size_t k_bytes = (size_t)nk * m->dim * sizeof(double), h_bytes = (size_t)nk * nn2 * sizeof(double);
        const size_t p_bytes = convention == 1 ? (size_t)m->n_orb * m->dim * sizeof(double) : 0;
        const size_t h_off = (k_bytes + p_bytes + 63) / 64 * 64;  // (16-byte stores of H: keep the block aligned)
        if (m->h_stage != nullptr && h_off + h_bytes <= m->h_stage_bytes) {
            // small result (one k-point: 64 KiB of H at 64 orbitals): [k | pos | H] through the pinned buffer.  The chunked
            // download below -- a blocking copy into pageable memory -- takes 290 us per call for results of 25 - 64 KiB
            // in a loop of one-k calls (tools/trace_single_k.py), this path 50 - 95 us whatever the size
            char* st = static_cast<char*>(m->h_stage.h);
            TBK_CHECK(m->ws_k.reserve(k_bytes));
            TBK_CHECK(m->ws_out.reserve(h_bytes));
            // ONE k-point of a dense model (the Z2Pack call shape): k goes into the kernel arguments and the positions of
            // convention 1 stay on the device from call to call -- two uploads and one launch less per call
            const bool inline_k = nk == 1 && tbk_hk_plan(m, tbk_staged_operand(m), 1, false).rows == HK_ROWS_NONE;
            const double* d_pos = nullptr;
            tbk_one_k_t one_k;
            if (inline_k) {
                if (convention == 1) {
                    const size_t n_pos = (size_t)m->n_orb * m->dim;
                    if (m->pos_cache.size() != n_pos || std::memcmp(m->pos_cache.data(), pos, p_bytes) != 0) {
                        TBK_CHECK(m->ws_posraw.reserve(p_bytes));
                        std::memcpy(st + k_bytes, pos, p_bytes);
                        TBK_HIP(hipMemcpyAsync(m->ws_posraw.ptr, st + k_bytes, p_bytes, hipMemcpyHostToDevice, m->stream));
                        m->pos_cache.assign(pos, pos + n_pos);
                    }
                    one_k.d_pos_raw = m->ws_posraw.as<double>();
                }
                one_k.h_k = k;
            } else {
                std::memcpy(st, k, k_bytes);
                TBK_HIP(hipMemcpyAsync(m->ws_k.ptr, st, k_bytes, hipMemcpyHostToDevice, m->stream));
                if (convention == 1) {
                    TBK_CHECK(m->ws_pos.reserve(p_bytes));
                    std::memcpy(st + k_bytes, pos, p_bytes);
                    TBK_HIP(hipMemcpyAsync(m->ws_pos.ptr, st + k_bytes, p_bytes, hipMemcpyHostToDevice, m->stream));
                    d_pos = m->ws_pos.as<double>();
                }
            }
            // Round 6: up to 1 MiB of H the kernels store straight into the pinned buffer (a host allocation is
            // device-addressable; the stores collect in the L2 and leave with the system-scope release of ev_sync) -- no
            // copy kernel and no dependent boundary in front of it: one-k hamilton 84 -> 68 us at 64 orbitals, 124 -> 112
            // at 256 (sparse).  4 MiB (512 orbitals) written that way take longer than the copy (scattered 16-byte stores
            // across PCIe: 1.69 -> 1.81 ms), so a bigger H still takes the copy; downloading it in two or four pieces, each
            // copied on to the caller's array while the next crosses PCIe, was measured and is within the noise of the
            // 1.3 - 1.4 ms kernel in front of it (1586 / 1661 / 1704 and 1568 / 1613 / 1563 us for 1 / 2 / 4 pieces).
            constexpr size_t ZERO_COPY_MAX = size_t(1) << 20;
            const bool direct = h_bytes <= ZERO_COPY_MAX;
            double* d_out = direct ? reinterpret_cast<double*>(st + h_off) : m->ws_out.as<double>();
            TBK_CHECK(hamilton_chunks(m, m->ws_k.as<double>(), nk, convention, d_pos, one_k, d_out));
            if (!direct) TBK_HIP(hipMemcpyAsync(st + h_off, m->ws_out.ptr, h_bytes, hipMemcpyDeviceToHost, m->stream));
            TBK_CHECK(wait_main_stream(m));
            std::memcpy(H_out, st + h_off, h_bytes);
            return TBK_OK;
        }
    }
    // H leaves in chunks of 16 to 128 MiB (a quarter of the result) through two device buffers: chunk c + 1 is computed while chunk c crosses PCIe
    // (the copy into pageable memory blocks this thread, not the GPU)
    const size_t total_bytes = (size_t)nk * nn2 * sizeof(double);
    const size_t chunk_bytes = std::min<size_t>(size_t(128) << 20, std::max<size_t>(size_t(16) << 20, total_bytes / 4));
    int64_t out_chunk = std::max<int64_t>(1, (int64_t)(chunk_bytes / (nn2 * sizeof(double))));
    out_chunk = std::min(out_chunk, nk);
    const int64_t n_chunks = (nk + out_chunk - 1) / out_chunk;
    TBK_CHECK(m->ws_k.reserve((size_t)nk * m->dim * sizeof(double)));
    TBK_HIP(hipMemcpyAsync(m->ws_k.ptr, k, (size_t)nk * m->dim * sizeof(double), hipMemcpyHostToDevice, m->stream));
    const double* d_pos = nullptr;
    if (convention == 1) {
        TBK_CHECK(m->ws_pos.reserve((size_t)m->n_orb * m->dim * sizeof(double)));
        TBK_HIP(hipMemcpyAsync(m->ws_pos.ptr, pos, (size_t)m->n_orb * m->dim * sizeof(double),
                               hipMemcpyHostToDevice, m->stream));
        d_pos = m->ws_pos.as<double>();
    }
    DevBuf* obuf[2] = {&m->ws_out, &m->ws_out2};
    for (int b = 0; b < (n_chunks > 1 ? 2 : 1); ++b) TBK_CHECK(obuf[b]->reserve((size_t)out_chunk * nn2 * sizeof(double)));
    auto compute = [&](int64_t c) -> int {
        const int64_t c0 = c * out_chunk, nkc = std::min(out_chunk, nk - c0);
        TBK_CHECK(hamilton_chunks(m, m->ws_k.as<double>() + c0 * m->dim, nkc, convention, d_pos, tbk_one_k_t(), obuf[c & 1]->as<double>()));
        TBK_HIP(hipEventRecord(m->ev_out[c & 1], m->stream));
        return TBK_OK;
    };
    TBK_CHECK(compute(0));
    for (int64_t c = 0; c < n_chunks; ++c) {
        const int64_t c0 = c * out_chunk, nkc = std::min(out_chunk, nk - c0);
        if (c + 1 < n_chunks) TBK_CHECK(compute(c + 1));  // its buffer was drained by the (blocking) copy of chunk c - 1
        TBK_HIP(hipEventSynchronize(m->ev_out[c & 1]));
        TBK_HIP(hipMemcpy(H_out + (size_t)c0 * nn2, obuf[c & 1]->ptr, (size_t)nkc * nn2 * sizeof(double), hipMemcpyDeviceToHost));
    }
    return wait_main_stream(m);
}

// Small eigenvalue calls: the eigenvalues AND the two flag words leave the device through ONE small kernel that stores them
// straight into the pinned buffer (device-addressable host memory; the stores leave with the system-scope release of ev_sync).
// They used to be two hipMemcpyAsync, i.e. two copy kernels of ~4.4 us each with a dependent boundary in front of each: 8.8 of
// the 33 us of GPU work of a one-k eigenval of the silicon model.
__global__ void __launch_bounds__(256) export_small_kernel(const double* __restrict__ E, int64_t count, const int* __restrict__ flag,
                                                           double* __restrict__ host_E, int* __restrict__ host_flag) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) host_E[i] = E[i];
    if (blockIdx.x == 0 && threadIdx.x < 2) host_flag[threadIdx.x] = flag[threadIdx.x];
}

extern "C" int tbk_eigenval(tbk_model* m, const double* k, int64_t nk, double* E_out) {
    TBK_ARG(m != nullptr, "model is NULL");
    TBK_LOCK(m);
    TBK_ARG(nk >= 0, "nk < 0");
    if (nk == 0) return TBK_OK;
    TBK_ARG(k && E_out, "k / E is NULL");
    TBK_HIP(hipSetDevice(m->device));
    const tbk_eig_plan_t plan = tbk_eig_plan(m->n_orb, m->eigensolver, nk);
    const size_t k_bytes = (size_t)nk * m->dim * sizeof(double), e_bytes = (size_t)nk * m->n_orb * sizeof(double);
    TBK_CHECK(m->ws_k.reserve(k_bytes));
    TBK_CHECK(m->ws_out.reserve(e_bytes));
    const size_t e_off = (k_bytes + 63) / 64 * 64;
    if (m->h_stage != nullptr && e_off + e_bytes + 16 <= m->h_stage_bytes) {
        // small call: [k | E | flags] through the pinned buffer, everything enqueued, one synchronisation
        char* st = static_cast<char*>(m->h_stage.h);
        int* flag = reinterpret_cast<int*>(st + e_off + e_bytes);
        // (one k-point of a dense model on the matrix-vector path: k travels in the kernel arguments, see tbk_hamilton --
        // only the chunk pipeline reads it from there: the rocSOLVER branch fills its phase rows from ws_k, which a call
        // that skipped the upload would leave stale)
        const bool inline_k = nk == 1 && plan.own() && tbk_hk_plan(m, tbk_staged_operand(m), 1, false).rows == HK_ROWS_NONE;
        const tbk_one_k_t one_k = {inline_k ? k : nullptr, nullptr};
        if (!inline_k) {
            std::memcpy(st, k, k_bytes);
            TBK_HIP(hipMemcpyAsync(m->ws_k.ptr, st, k_bytes, hipMemcpyHostToDevice, m->stream));
        }
        // (the eigenvalues stored straight into the pinned buffer, like H in tbk_hamilton: measured, no gain -- 180.2 vs 180.0 us)
        TBK_CHECK(eigenval_device_impl(m, plan, m->ws_k.as<double>(), k, nk, m->ws_out.as<double>(), one_k, nullptr));
        {
            const int64_t count = nk * m->n_orb;
            const unsigned blocks = (unsigned)std::min<int64_t>((count + 255) / 256, 64);
            hipLaunchKernelGGL(export_small_kernel, dim3(blocks), dim3(256), 0, m->stream, m->ws_out.as<double>(), count,
                               m->ws_flag.as<int>(), reinterpret_cast<double*>(st + e_off), flag);
            TBK_HIP(hipGetLastError());
        }
        TBK_CHECK(wait_main_stream(m));
        std::memcpy(E_out, st + e_off, e_bytes);
        if (flag[0] != 0 || flag[1] != 0) return tbk_eigenval_check(m);  // (rare) the ordinary path reports and resets
        return TBK_OK;
    }
    TBK_HIP(hipMemcpyAsync(m->ws_k.ptr, k, k_bytes, hipMemcpyHostToDevice, m->stream));
    TBK_CHECK(eigenval_device_impl(m, plan, m->ws_k.as<double>(), k, nk, m->ws_out.as<double>(), tbk_one_k_t(), nullptr));
    TBK_HIP(hipMemcpyAsync(E_out, m->ws_out.ptr, e_bytes, hipMemcpyDeviceToHost, m->stream));
    return tbk_eigenval_check(m);  // synchronises
}

// ------------------------------------------------------------------------------------------------
// the reduction stage alone, on caller-supplied matrices
// ------------------------------------------------------------------------------------------------
extern "C" int tbk_tridiagonal_reduce(int device, int n_orb, int64_t nk, const double* H, int method, double* d, double* e,
                                      double* H_reduced) {
    TBK_ARG(nk >= 0, "nk < 0");
    TBK_ARG(n_orb >= 1 && (n_orb <= 64 || tbk_eig_band_supported(n_orb)),
            "n_orb must be in [1, 4096] (larger matrices go through rocSOLVER as a whole)");
    TBK_ARG(method >= TBK_REDUCE_AUTO && method <= TBK_REDUCE_TWO_STAGE, "unknown reduction method");
    TBK_ARG(method != TBK_REDUCE_TWO_STAGE || tbk_eig_band_supported(n_orb), "the two-stage reduction handles 64 < n_orb <= 4096");
    TBK_ARG(method != TBK_REDUCE_ONE_STAGE || n_orb <= 512, "the one-stage reduction handles n_orb <= 512");
    if (nk == 0) return TBK_OK;
    TBK_ARG(H && d && e, "H / d / e is NULL");
    ModelGuard guard;  // (declared in front of the lock: destroyed behind it)
    TBK_CHECK(create_common(device, 1, n_orb, 0, nullptr, 2, false, &guard));
    tbk_model* m = guard.get();
    const size_t n = (size_t)n_orb, mat_bytes = n * n * 2 * sizeof(double);
    TBK_LOCK(m);
    const tbk_eig_plan_t plan = tbk_eig_plan(n_orb, m->eigensolver, nk, method);
    TBK_CHECK(m->ws_H.reserve((size_t)nk * mat_bytes));
    TBK_CHECK(m->ws_E.reserve((size_t)nk * n * 2 * sizeof(double)));
    TBK_CHECK(tbk_eig_reserve(m, plan, nk, 1));
    TBK_HIP(hipMemcpyAsync(m->ws_H.ptr, H, (size_t)nk * mat_bytes, hipMemcpyHostToDevice, m->stream));
    TBK_CHECK(tbk_eig_reduce(m, plan, m->stream, m->ws_H.as<double>(), nk, m->ws_E.as<double>()));
    TBK_HIP(hipMemcpyAsync(d, m->ws_E.ptr, (size_t)nk * n * sizeof(double), hipMemcpyDeviceToHost, m->stream));
    TBK_HIP(hipMemcpyAsync(e, m->ws_E.as<double>() + (size_t)nk * n, (size_t)nk * n * sizeof(double), hipMemcpyDeviceToHost,
                           m->stream));
    if (H_reduced)
        TBK_HIP(hipMemcpyAsync(H_reduced, m->ws_H.ptr, (size_t)nk * mat_bytes, hipMemcpyDeviceToHost, m->stream));
    TBK_HIP(hipStreamSynchronize(m->stream));
    return TBK_OK;
}

// The reduction stage ALONE on the chip, timed with HIP events: what `eig_roofline.standalone` of bench.py quotes beside the
// in-pipeline figure (there the H(k) of the next chunk shares the FP64 pipe).  Random Hermitian matrices are made on the
// device; every repetition works on a fresh copy (the reduction consumes its input), only the reduction is inside the events.
__global__ void __launch_bounds__(256) random_hermitian_kernel(double* __restrict__ H, int n, int64_t nk) {
    const int64_t total = nk * (int64_t)n * n;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        const int64_t mat = t / ((int64_t)n * n);
        const int r = (int)((t / n) % n), c = (int)(t % n);
        const int i = r < c ? r : c, j = r < c ? c : r;  // the element of the upper triangle this one mirrors
        uint64_t x = (uint64_t)mat * 0x9E3779B97F4A7C15ull + (uint64_t)i * 0xBF58476D1CE4E5B9ull + (uint64_t)j * 0x94D049BB133111EBull + 1;
        x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
        const double re = (double)(int64_t)(x >> 11) * (1.0 / 9007199254740992.0) - 0.5;
        x ^= x >> 29; x *= 0x9E3779B97F4A7C15ull; x ^= x >> 32;
        const double im = (double)(int64_t)(x >> 11) * (1.0 / 9007199254740992.0) - 0.5;
        H[2 * t] = re;
        H[2 * t + 1] = i == j ? 0.0 : (r < c ? im : -im);
    }
}

extern "C" int tbk_reduce_standalone(int device, int n_orb, int64_t nk, int reps, double* us_per_matrix) {
    TBK_ARG(us_per_matrix != nullptr, "us_per_matrix is NULL");
    TBK_ARG(nk >= 1 && reps >= 1, "nk / reps < 1");
    TBK_ARG(n_orb >= 1 && (n_orb <= 64 || tbk_eig_band_supported(n_orb)), "n_orb must be in [1, 4096]");
    for (int q = 0; q < 3; ++q) us_per_matrix[q] = 0.0;
    ModelGuard guard;  // (declared in front of the lock: destroyed behind it)
    TBK_CHECK(create_common(device, 1, n_orb, 0, nullptr, 2, false, &guard));
    tbk_model* m = guard.get();
    const size_t n = (size_t)n_orb, mat_bytes = n * n * 2 * sizeof(double);
    DevBuf pristine;
    Event ev[2];
    TBK_LOCK(m);
    const tbk_eig_plan_t plan = tbk_eig_plan(n_orb, m->eigensolver, nk);
    TBK_CHECK(pristine.reserve((size_t)nk * mat_bytes));
    TBK_CHECK(m->ws_H.reserve((size_t)nk * mat_bytes));
    TBK_CHECK(m->ws_E.reserve((size_t)nk * n * 2 * sizeof(double)));
    TBK_HIP(hipEventCreate(ev[0].put()));
    TBK_HIP(hipEventCreate(ev[1].put()));
    hipLaunchKernelGGL(random_hermitian_kernel, dim3(4096), dim3(256), 0, m->stream, pristine.as<double>(), n_orb, nk);
    TBK_HIP(hipGetLastError());
    const bool band = plan.family == EIG_TWO_STAGE;
    TBK_CHECK(tbk_eig_reserve(m, plan, nk, 1));
    // (the stages run apart below at every two-stage size, a band buffer between them also where the plan fuses them)
    TBK_CHECK(m->ws_bandmat[0].reserve((size_t)nk * plan.band_stride));
    // what: 0 = the reduction as the pipeline runs it, 1 = first stage alone, 2 = second stage alone (two-stage sizes only).
    // The second stage has no input of its own: every repetition of `what == 2` chases the band the LAST repetition of
    // `what == 1` left in ws_bandmat[0] (the chase reads it and writes only (d, e): the same work every time).
    for (int what = 0; what < (band ? 3 : 1); ++what) {
        float sum = 0.0f;
        for (int r = 0; r <= reps; ++r) {  // (repetition 0 warms up)
            if (what != 2)
                TBK_HIP(hipMemcpyAsync(m->ws_H.ptr, pristine.ptr, (size_t)nk * mat_bytes, hipMemcpyDeviceToDevice, m->stream));
            TBK_HIP(hipEventRecord(ev[0], m->stream));
            if (what == 0) {
                TBK_CHECK(tbk_eig_reduce(m, plan, m->stream, m->ws_H.as<double>(), nk, m->ws_E.as<double>()));
            } else if (what == 1) {
                TBK_CHECK(tbk_launch_band_reduce(m, plan, m->stream, m->ws_H.as<double>(), nk, m->ws_band.ptr, m->ws_bandmat[0].ptr));
            } else {
                TBK_CHECK(tbk_launch_band_chase(m, plan, m->stream, m->ws_bandmat[0].ptr, nk, m->ws_E.as<double>()));
            }
            TBK_HIP(hipEventRecord(ev[1], m->stream));
            TBK_HIP(hipEventSynchronize(ev[1]));
            float ms = 0.0f;
            TBK_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
            if (r > 0) sum += ms;
        }
        us_per_matrix[what] = (double)sum / reps * 1e3 / (double)nk;
    }
    return TBK_OK;
}

// ------------------------------------------------------------------------------------------------
// k.p models
// ------------------------------------------------------------------------------------------------
extern "C" int tbk_kdotp_create(int device, int dim, int n_orb, int64_t n_p, const int32_t* powers,
                                const double* coeffs, tbk_kdotp** out) {
    TBK_ARG(out != nullptr, "out is NULL");
    *out = nullptr;
    TBK_ARG(n_p == 0 || (powers && coeffs), "powers / coeffs is NULL");
    for (int64_t t = 0; t < n_p * dim; ++t) TBK_ARG(powers[t] >= 0, "negative power");
    ModelGuard guard;
    TBK_CHECK(create_common(device, dim, n_orb, n_p, nullptr, 1, false, &guard));
    tbk_model* m = guard.get();
    m->kdotp = true;
    DevPtr<double> d_raw;
    const size_t raw_bytes = (size_t)n_p * n_orb * n_orb * 2 * sizeof(double);
    if (n_p > 0) {
        TBK_HIP(hipMalloc(m->d_powers.put(), (size_t)n_p * dim * sizeof(int32_t)));
        TBK_HIP(hipMemcpy(m->d_powers, powers, (size_t)n_p * dim * sizeof(int32_t), hipMemcpyHostToDevice));
        TBK_HIP(hipMalloc(d_raw.put(), raw_bytes));
        TBK_HIP(hipMemcpyAsync(d_raw, coeffs, raw_bytes, hipMemcpyHostToDevice, m->stream));
    }
    TBK_CHECK(tbk_stage_kdotp(m, d_raw));
    TBK_HIP(hipStreamSynchronize(m->stream));
    tbk_kdotp* kp = new (std::nothrow) tbk_kdotp();
    if (!kp) {
        tbk_set_error("out of host memory");
        return TBK_ERR_MEMORY;
    }
    kp->core = guard.release();
    *out = kp;
    return TBK_OK;
}

extern "C" void tbk_kdotp_destroy(tbk_kdotp* kp) {
    if (!kp) return;
    tbk_model_destroy(kp->core);
    delete kp;
}

extern "C" int tbk_kdotp_hamilton(tbk_kdotp* kp, const double* k, int64_t nk, double* H_out) {
    TBK_ARG(kp != nullptr, "model is NULL");
    return tbk_hamilton(kp->core, k, nk, 2, nullptr, H_out);
}

extern "C" int tbk_kdotp_eigenval(tbk_kdotp* kp, const double* k, int64_t nk, double* E_out) {
    TBK_ARG(kp != nullptr, "model is NULL");
    return tbk_eigenval(kp->core, k, nk, E_out);
}

// ------------------------------------------------------------------------------------------------
// device memory helpers
// ------------------------------------------------------------------------------------------------
extern "C" int tbk_device_malloc(int device, int64_t bytes, void** d_ptr) {
    TBK_ARG(d_ptr != nullptr && bytes >= 0, "bad malloc arguments");
    TBK_CHECK(require_device(device));
    *d_ptr = nullptr;
    if (bytes == 0) return TBK_OK;
    TBK_HIP(hipMalloc(d_ptr, (size_t)bytes));
    return TBK_OK;
}

extern "C" int tbk_device_free(int device, void* d_ptr) {
    if (!d_ptr) return TBK_OK;
    TBK_CHECK(require_device(device));
    TBK_HIP(hipFree(d_ptr));
    return TBK_OK;
}

extern "C" int tbk_memcpy_h2d(int device, void* d_dst, const void* h_src, int64_t bytes) {
    TBK_CHECK(require_device(device));
    if (bytes > 0) {
        TBK_HIP(hipMemcpy(d_dst, h_src, (size_t)bytes, hipMemcpyHostToDevice));
        TBK_HIP(hipDeviceSynchronize());  // pageable H2D may return before the DMA has landed
    }
    return TBK_OK;
}

extern "C" int tbk_memcpy_d2h(int device, void* h_dst, const void* d_src, int64_t bytes) {
    TBK_CHECK(require_device(device));
    if (bytes > 0) TBK_HIP(hipMemcpy(h_dst, d_src, (size_t)bytes, hipMemcpyDeviceToHost));
    return TBK_OK;
}

extern "C" int tbk_device_mem_info(int device, int64_t* free_bytes, int64_t* total_bytes) {
    TBK_CHECK(require_device(device));
    size_t f = 0, t = 0;
    TBK_HIP(hipMemGetInfo(&f, &t));
    if (free_bytes) *free_bytes = (int64_t)f;
    if (total_bytes) *total_bytes = (int64_t)t;
    return TBK_OK;
}

// ------------------------------------------------------------------------------------------------
// timing
// ------------------------------------------------------------------------------------------------
extern "C" int tbk_get_timing(tbk_model* m, double* ms, int64_t* launches, int reset) {
    TBK_ARG(m != nullptr, "model is NULL");
    TBK_LOCK(m);
    TBK_HIP(hipSetDevice(m->device));
    TBK_HIP(hipStreamSynchronize(m->stream));
    TBK_HIP(hipStreamSynchronize(m->stream_eig));
    TBK_HIP(hipStreamSynchronize(m->stream_ql));
    for (const EventSpan& ev : m->events) {
        float t = 0.f;
        if (hipEventElapsedTime(&t, ev.start, ev.stop) == hipSuccess) {
            m->t_ms[ev.stage] += (double)t;
            m->t_n[ev.stage] += 1;
        }
    }
    m->events.clear();
    for (int i = 0; i < TBK_T_COUNT; ++i) {
        if (ms) ms[i] = m->t_ms[i];
        if (launches) launches[i] = m->t_n[i];
        if (reset) {
            m->t_ms[i] = 0.0;
            m->t_n[i] = 0;
        }
    }
    return TBK_OK;
}

extern "C" int tbk_mfma_f64_peak(int device, double* tflops) {
    TBK_ARG(tflops != nullptr, "tflops is NULL");
    TBK_CHECK(require_device(device));
    return tbk_run_mfma_f64_peak(tflops);
}
