// tbk_fold.hip -- k lists with long runs of a shared component (uniform grids, planes, lines): fold the model
// along that component once per run and evaluate a model of lower dimension.
//
// The Fourier sum of /root/reference/src/tbmodels/_tb_model.py:1109-1122 costs 8 N^2 N_R flops per k-point
// whatever the k list looks like.  On a grid -- BASELINE config 4 is the 100 x 100 x 100 mesh of
// `np.meshgrid(..., indexing="ij")` -- 10^4 consecutive k-points share k_1, and for them
//
//     exp(2 pi i k.R) = exp(2 pi i k_1 R_1) * exp(2 pi i (k_2 R_2 + k_3 R_3))
//
// so the lattice vectors that differ only in R_1 can be summed ONCE per plane:
//
//     hop'[(R_2, R_3)] = sum_{R_1} exp(2 pi i k_1 R_1) hop[(R_1, R_2, R_3)]
//
// and the plane is a 2-D model with as many "lattice vectors" as there are distinct (R_2, R_3): 313 instead of
// 4096 half-space vectors for the synthetic headline model (|R_i| <= 12) -- 13x less work for the H(k) contraction,
// with every kernel of the path unchanged (phase rows, MFMA contraction, eigensolvers all run on the folded model).
//
// The fold acts on an operand Bt (two real rows P_r, Q_r per lattice vector: H = sum_r c_r P_r + s_r Q_r, tbk_stage.hip) --
// a tbk_operand_t: the staged one, or, for the mesh lines inside a plane, a folded one.  With theta = alpha + sigma beta' (alpha = 2 pi k_f R_f, beta' the phase of the canonical
// (dim-1)-vector rho', sigma = -1 where R's remaining components had to be negated to make them canonical):
//
//     P'_rho += cos(alpha) P_r + sin(alpha) Q_r          Q'_rho += sigma (-sin(alpha) P_r + cos(alpha) Q_r)
//
// One pass over Bt per run (272 MB at the headline shape: 55 us) against a contraction 13x shorter.
//
// Kernels and plans first, then the host analysis of a k list (no model, no device), then the driver of one folded
// eigenvalue call (tbk_folded_call), whose build() the chunk pipeline of tbk_api.hip runs.

#include <algorithm>
#include <cstring>
#include <map>
#include <vector>

#include "tbk_internal.h"

namespace {

// thread (column c of the flattened Bt row, folded vector rho): gathers the rows of its list
__global__ void __launch_bounds__(256)
fold_rows_kernel(const double* __restrict__ Bt, int64_t row_len, const int64_t* __restrict__ lptr,
                 const int32_t* __restrict__ lrec, const int32_t* __restrict__ rcomp, double k_f,
                 double* __restrict__ B2) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t rho = blockIdx.y;
    if (c >= row_len) return;
    double accp = 0.0, accq = 0.0;
    for (int64_t t = lptr[rho]; t < lptr[rho + 1]; ++t) {
        const int32_t rec = lrec[t];
        const int64_t r = rec & 0x7fffffff;
        const double sigma = rec < 0 ? -1.0 : 1.0;
        double sa, ca;
        sincospi(2.0 * k_f * (double)rcomp[r], &sa, &ca);  // uniform per (rho, t): exact argument reduction
        const double p = Bt[(2 * r) * row_len + c], q = Bt[(2 * r + 1) * row_len + c];
        accp = fma(ca, p, fma(sa, q, accp));
        accq = fma(sigma * ca, q, fma(-sigma * sa, p, accq));
    }
    B2[(2 * rho) * row_len + c] = accp;
    B2[(2 * rho + 1) * row_len + c] = accq;
}

constexpr int FOLD_GROUP = 16;

struct FoldValues {
    double v[FOLD_GROUP];  // shared-component value of every run of the group (a kernel argument: no copy to wait for)
};

// (cos, sin)(2 pi k_f[g] R_f[r]) for the runs of a group
__global__ void fold_table_kernel(const int32_t* __restrict__ rcomp, int64_t n_r, const FoldValues k_f, int n_g,
                                  double* __restrict__ table) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_r * n_g) return;
    const int64_t r = i / n_g;
    const int g = (int)(i % n_g);
    double sa, ca;
    sincospi(2.0 * k_f.v[g] * (double)rcomp[r], &sa, &ca);  // exact argument reduction
    table[2 * i] = ca;
    table[2 * i + 1] = sa;
}

// the same table for n_g lines whose shared-component values sit in device memory at k_f[g * stride]
__global__ void fold_table_dev_kernel(const int32_t* __restrict__ rcomp, int64_t n_r, const double* __restrict__ k_f,
                                      int64_t stride, int n_g, double* __restrict__ table) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_r * n_g) return;
    const int64_t r = i / n_g;
    const int g = (int)(i % n_g);
    double sa, ca;
    sincospi(2.0 * k_f[(int64_t)g * stride] * (double)rcomp[r], &sa, &ca);
    table[2 * i] = ca;
    table[2 * i + 1] = sa;
}

// The same fold for up to FOLD_GROUP runs in ONE pass over Bt: every (row pair, column) is loaded once and
// accumulated into the operand of each run of the group (its phases come from the table above).

__global__ void __launch_bounds__(256)
fold_rows_group_kernel(const double* __restrict__ Bt, int64_t row_len, const int64_t* __restrict__ lptr,
                       const int32_t* __restrict__ lrec, const double* __restrict__ table_all, int n_total,
                       int64_t b2_stride, double* __restrict__ B2_all) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t rho = blockIdx.y;
    if (c >= row_len) return;
    // blockIdx.z: which FOLD_GROUP slots of the n_total this block folds
    const int g_base = blockIdx.z * FOLD_GROUP;
    const int n_g = min(FOLD_GROUP, n_total - g_base);
    const double* table = table_all + 2 * g_base;
    double* B2 = B2_all + (size_t)g_base * b2_stride;
    double accp[FOLD_GROUP], accq[FOLD_GROUP];
#pragma unroll
    for (int g = 0; g < FOLD_GROUP; ++g) accp[g] = accq[g] = 0.0;
    for (int64_t t = lptr[rho]; t < lptr[rho + 1]; ++t) {
        const int32_t rec = lrec[t];
        const int64_t r = rec & 0x7fffffff;
        const double sigma = rec < 0 ? -1.0 : 1.0;
        const double p = Bt[(2 * r) * row_len + c], q = Bt[(2 * r + 1) * row_len + c];
        const double* tab = table + 2 * r * n_total;  // uniform
#pragma unroll
        for (int g = 0; g < FOLD_GROUP; ++g) {
            if (g < n_g) {
                const double ca = tab[2 * g], sa = tab[2 * g + 1];
                accp[g] = fma(ca, p, fma(sa, q, accp[g]));
                accq[g] = fma(sigma * ca, q, fma(-sigma * sa, p, accq[g]));
            }
        }
    }
#pragma unroll
    for (int g = 0; g < FOLD_GROUP; ++g) {
        if (g < n_g) {
            B2[g * b2_stride + (2 * rho) * row_len + c] = accp[g];
            B2[g * b2_stride + (2 * rho + 1) * row_len + c] = accq[g];
        }
    }
}

// k2[i][:] = k[i][all components but f]
__global__ void drop_component_kernel(const double* __restrict__ k, int dim, int f, int64_t nk, double* __restrict__ k2) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nk) return;
    int o = 0;
    for (int d = 0; d < dim; ++d)
        if (d != f) k2[i * (dim - 1) + o++] = k[i * dim + d];
}

bool canonical_negate(std::vector<int32_t>& v) {
    for (int32_t x : v) {
        if (x > 0) return false;
        if (x < 0) {
            for (int32_t& y : v) y = -y;
            return true;
        }
    }
    return false;
}

}  // namespace

// Builds the folded lattice and the row lists for folding the lattice R[n_r][dim] along component f.
static int build_plan(tbk_fold_plan_t& plan, const int32_t* R, int64_t n_r, int dim, int f, int ncol_pad, int capacity) {
    if (plan.built) return TBK_OK;
    std::map<std::vector<int32_t>, int32_t> index;
    std::vector<std::vector<int32_t>> lists;
    std::vector<int32_t> rcomp((size_t)n_r);
    plan.h_R2.clear();
    for (int64_t r = 0; r < n_r; ++r) {
        std::vector<int32_t> rho;
        for (int d = 0; d < dim; ++d)
            if (d != f) rho.push_back(R[(size_t)r * dim + d]);
        rcomp[(size_t)r] = R[(size_t)r * dim + f];
        const bool negated = canonical_negate(rho);
        auto it = index.find(rho);
        if (it == index.end()) {
            it = index.emplace(rho, (int32_t)lists.size()).first;
            lists.emplace_back();
            plan.h_R2.insert(plan.h_R2.end(), rho.begin(), rho.end());
        }
        lists[(size_t)it->second].push_back((int32_t)r | (negated ? (int32_t)0x80000000 : 0));
    }
    plan.dim = dim;
    plan.n_r = n_r;
    plan.n_rho = (int64_t)lists.size();
    plan.k2 = (plan.n_rho * 2 + TBK_BK - 1) / TBK_BK * TBK_BK;
    plan.n_rho_pad = plan.k2 / 2;
    plan.capacity = capacity;
    plan.row_len = (int64_t)ncol_pad * 2;
    std::vector<int64_t> lptr((size_t)plan.n_rho_pad + 1, 0);
    std::vector<int32_t> lrec;
    for (int64_t i = 0; i < plan.n_rho_pad; ++i) {
        if (i < plan.n_rho) lrec.insert(lrec.end(), lists[(size_t)i].begin(), lists[(size_t)i].end());
        lptr[(size_t)i + 1] = (int64_t)lrec.size();  // padding vectors keep empty lists: zero rows
    }
    std::vector<int32_t> r2((size_t)plan.n_rho_pad * std::max(dim - 1, 1), 0);
    std::copy(plan.h_R2.begin(), plan.h_R2.end(), r2.begin());
    TBK_HIP(hipMalloc(plan.d_R2.put(), std::max<size_t>(r2.size(), 1) * sizeof(int32_t)));
    TBK_HIP(hipMalloc(plan.d_lptr.put(), lptr.size() * sizeof(int64_t)));
    TBK_HIP(hipMalloc(plan.d_lrec.put(), std::max<size_t>(lrec.size(), 1) * sizeof(int32_t)));
    TBK_HIP(hipMalloc(plan.d_rcomp.put(), std::max<size_t>(rcomp.size(), 1) * sizeof(int32_t)));
    TBK_HIP(hipMalloc(plan.d_B2.put(), (size_t)capacity * plan.k2 * plan.row_len * sizeof(double)));
    plan.table_entries = n_r * FOLD_GROUP;
    TBK_HIP(hipMalloc(plan.d_table.put(), std::max<size_t>((size_t)plan.table_entries * 2, 1) * sizeof(double)));
    TBK_HIP(hipMemcpy(plan.d_R2, r2.data(), r2.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    TBK_HIP(hipMemcpy(plan.d_lptr, lptr.data(), lptr.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    TBK_HIP(hipMemcpy(plan.d_lrec, lrec.data(), lrec.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    TBK_HIP(hipMemcpy(plan.d_rcomp, rcomp.data(), rcomp.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    plan.built = true;
    return TBK_OK;
}

static int tbk_fold_plan(tbk_model* m, int f) {
    return build_plan(m->fold[f], m->h_R.data(), m->n_r, m->dim, f, m->ncol_pad, FOLD_GROUP);
}

// Second-level plan: folds the lattice `parent` produced along its component f2 (mesh lines inside a mesh plane);
// room for `capacity` operands (one per line of a plane piece).
static int tbk_fold_subplan(tbk_model* m, tbk_fold_plan_t& parent, int f2, int capacity, tbk_fold_plan_t** out) {
    *out = nullptr;
    const int dim2 = parent.dim - 1;
    if (dim2 < 2 || f2 < 0 || f2 >= dim2) return TBK_OK;
    if (!parent.sub) parent.sub.reset(new tbk_fold_plan_t[TBK_MAX_DIM]);
    tbk_fold_plan_t& plan = parent.sub[f2];
    if (plan.built && plan.capacity < capacity) plan = tbk_fold_plan_t();  // a longer piece than any before: rebuild with more room
    TBK_CHECK(build_plan(plan, parent.h_R2.data(), parent.n_rho, dim2, f2, m->ncol_pad, capacity));
    *out = &plan;
    return TBK_OK;
}

// Average run length from which folding pays: a run costs one pass over Bt (60 us at the headline shape) plus
// three small launches, the direct contraction ~1 us per k-point.  Measured on meshes of the headline model:
// 14^3 (runs of 196) 4.4 -> 2.4 ms, 20^3 11.4 -> 5.0 ms, 30^3 38 -> 13.6 ms, 50^3 159 -> 49 ms.
static int64_t tbk_fold_min_run() { return 128; }

// Which component (if any) is worth folding for this k list: the one with the fewest runs of equal consecutive
// values, if its runs average >= tbk_fold_min_run() k-points and the folded lattice is at least 3x smaller.  -1: none.
static int tbk_fold_choose(tbk_model* m, const double* h_k, int64_t nk, std::vector<int64_t>& run_starts) {
    run_starts.clear();
    if (!m->fold_enabled || m->sparse || m->kdotp || m->dim < 2 || m->n_r < 64 || nk < 1024 || m->h_R.empty()) return -1;
    int best = -1;
    int64_t best_runs = nk;
    for (int d = 0; d < m->dim; ++d) {
        int64_t runs = 1;
        for (int64_t i = 1; i < nk && runs * tbk_fold_min_run() <= nk; ++i)
            if (h_k[i * m->dim + d] != h_k[(i - 1) * m->dim + d]) ++runs;
        if (runs * tbk_fold_min_run() <= nk && runs < best_runs) {
            best_runs = runs;
            best = d;
        }
    }
    if (best < 0) return -1;
    if (tbk_fold_plan(m, best) != TBK_OK) return -1;
    if (m->fold[best].n_rho * 3 > m->n_r) return -1;
    run_starts.push_back(0);
    for (int64_t i = 1; i < nk; ++i)
        if (h_k[i * m->dim + best] != h_k[(i - 1) * m->dim + best]) run_starts.push_back(i);
    run_starts.push_back(nk);
    return best;
}

// Chunks of a folded call: whole runs (mesh planes) packed up to the chunk size -- every run a chunk cuts costs a second
// fold pass, ragged mesh lines and a handful of small launches on both sides of the cut (the 100^3 mesh in chunks of 30 000
// = three planes instead of 32 768: 150.8 -> 143.6 ms).  Runs longer than a chunk are cut into chunk-sized pieces.
std::vector<int64_t> run_schedule(const std::vector<int64_t>& runs, int64_t chunk) {
    std::vector<int64_t> out;
    int64_t cur = 0;
    for (size_t r = 0; r + 1 < runs.size(); ++r) {
        int64_t len = runs[r + 1] - runs[r];
        if (cur > 0 && cur + len > chunk) {
            out.push_back(cur);
            cur = 0;
        }
        while (len > chunk) {
            out.push_back(chunk);
            len -= chunk;
        }
        cur += len;
    }
    if (cur > 0) out.push_back(cur);
    return out;
}

// Second level (meshes): inside a plane the k-points come in LINES -- equal-length sub-runs of one more shared
// component whose remaining coordinates repeat from line to line.  Every line is a (dim - 2)-dimensional model
// (13 instead of 313 lattice vectors at the headline shape); all lines of the piece go through ONE launch with
// per-line operands and shared phase rows (tbk_launch_hk_dense_lines).  Ragged ends of the piece, and anything
// that does not have this structure, take piece_plane.  The two functions that find the lines read the list of the call,
// h_k[.][dim]; reduced[e] is the original component of reduced component e of a run.

// equal remaining coordinates along the lines of L points that start at a0 and b0 (e2: the component shared along a line)
static bool same_line(const double* h_k, int dim, const std::vector<int>& reduced, int64_t a0, int64_t b0, int64_t L, int e2) {
    const int dim1 = (int)reduced.size();
    for (int64_t t = 0; t < L; ++t)
        for (int e = 0; e < dim1; ++e)
            if (e != e2 && h_k[(a0 + t) * dim + reduced[e]] != h_k[(b0 + t) * dim + reduced[e]]) return false;
    return true;
}

// the mesh lines of the piece [lo, hi) of one run
static LineInfo analyse(const double* h_k, int dim, const std::vector<int>& reduced, int64_t lo, int64_t hi) {
    const int dim1 = (int)reduced.size();
    LineInfo li;
    if (dim1 < 2 || hi - lo < 512) return li;
    // the reduced component with the longest sub-runs
    int e2 = -1;
    int64_t best_changes = hi - lo;
    for (int e = 0; e < dim1; ++e) {
        int64_t changes = 0;
        for (int64_t i = lo + 1; i < hi; ++i) changes += h_k[i * dim + reduced[e]] != h_k[(i - 1) * dim + reduced[e]];
        if (changes < best_changes) {
            best_changes = changes;
            e2 = e;
        }
    }
    if (e2 < 0 || best_changes < 4) return li;
    const int c2 = reduced[e2];
    std::vector<int64_t> sb(1, lo);  // sub-run starts
    for (int64_t i = lo + 1; i < hi; ++i)
        if (h_k[i * dim + c2] != h_k[(i - 1) * dim + c2]) sb.push_back(i);
    sb.push_back(hi);
    const size_t n_sub = sb.size() - 1;
    if (n_sub < 6) return li;
    const int64_t L = sb[2] - sb[1];  // an interior line
    if (L < 8 || L > TBK_BM) return li;
    // body: the longest prefix of interior sub-runs (from the second one) that are lines like the first of them
    size_t first = (sb[1] - sb[0] == L && same_line(h_k, dim, reduced, sb[0], sb[1], L, e2)) ? 0 : 1, last = first;
    while (last < n_sub && sb[last + 1] - sb[last] == L && same_line(h_k, dim, reduced, sb[first], sb[last], L, e2)) ++last;
    li.n_lines = (int64_t)(last - first);
    if (li.n_lines < 4) return li;
    li.ok = true;
    li.e2 = e2;
    li.L = L;
    li.body = sb[first];
    return li;
}

// Folds the operand `from` (the staged one, or a first-level folded one) for the n_g (<= FOLD_GROUP) shared-component
// values h_kf[] in one pass, into slots slot0 .. slot0 + n_g - 1 of the plan's buffer (main stream).
static int tbk_fold_group(tbk_model* m, const tbk_operand_t& from, tbk_fold_plan_t& plan, const double* h_kf, int n_g, int slot0) {
    const int64_t row_len = plan.row_len;
    double* out = plan.slot(slot0);
    StageTimer t(m, TBK_T_PHASE);
    if (n_g == 1) {
        dim3 grid((unsigned)((row_len + 255) / 256), (unsigned)plan.n_rho_pad);
        hipLaunchKernelGGL(fold_rows_kernel, grid, dim3(256), 0, m->stream, from.d_B, row_len, plan.d_lptr, plan.d_lrec,
                           plan.d_rcomp, h_kf[0], out);
        TBK_HIP(hipGetLastError());
        return TBK_OK;
    }
    FoldValues values;
    for (int g = 0; g < FOLD_GROUP; ++g) values.v[g] = g < n_g ? h_kf[g] : 0.0;
    const int64_t entries = plan.n_r * n_g;
    hipLaunchKernelGGL(fold_table_kernel, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, m->stream, plan.d_rcomp,
                       plan.n_r, values, n_g, plan.d_table);
    TBK_HIP(hipGetLastError());
    dim3 grid((unsigned)((row_len + 255) / 256), (unsigned)plan.n_rho_pad);
    hipLaunchKernelGGL(fold_rows_group_kernel, grid, dim3(256), 0, m->stream, from.d_B, row_len, plan.d_lptr, plan.d_lrec,
                       plan.d_table, n_g, plan.k2 * row_len, out);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

// All n_lines lines of a mesh plane piece in one go, folded from the operand `from` of their plane: their shared-component
// values are read on the device (d_kf[line * stride]); slots slot0 .. slot0 + n_lines - 1 of the plan's buffer
// (slot0 + n_lines <= plan.capacity).
static int tbk_fold_lines(tbk_model* m, const tbk_operand_t& from, tbk_fold_plan_t& plan, const double* d_kf, int64_t stride, int n_lines,
                          int slot0) {
    const int64_t row_len = plan.row_len;
    StageTimer t(m, TBK_T_PHASE);
    if ((size_t)plan.table_entries < (size_t)plan.n_r * n_lines) {
        plan.d_table.reset();
        plan.table_entries = plan.n_r * (int64_t)std::max(n_lines, plan.capacity);
        TBK_HIP(hipMalloc(plan.d_table.put(), std::max<size_t>((size_t)plan.table_entries * 2, 1) * sizeof(double)));
    }
    const int64_t entries = plan.n_r * n_lines;
    hipLaunchKernelGGL(fold_table_dev_kernel, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, m->stream,
                       plan.d_rcomp, plan.n_r, d_kf, stride, n_lines, plan.d_table);
    TBK_HIP(hipGetLastError());
    dim3 grid((unsigned)((row_len + 255) / 256), (unsigned)plan.n_rho_pad, (unsigned)((n_lines + FOLD_GROUP - 1) / FOLD_GROUP));
    hipLaunchKernelGGL(fold_rows_group_kernel, grid, dim3(256), 0, m->stream, from.d_B, row_len, plan.d_lptr, plan.d_lrec,
                       plan.d_table, n_lines, plan.k2 * row_len, plan.slot(slot0));
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

static int tbk_fold_drop_component(tbk_model* m, const double* d_k, int dim, int f, int64_t nk, double* d_k2) {
    hipLaunchKernelGGL(drop_component_kernel, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, m->stream, d_k, dim, f, nk,
                       d_k2);
    TBK_HIP(hipGetLastError());
    return TBK_OK;
}

// ------------------------------------------------------------------------------------------------
// the folded eigenvalue call
// ------------------------------------------------------------------------------------------------
constexpr int LINE_CAP = 512;  // lines per batch (operands: cap x k2'' x row)

tbk_folded_call::tbk_folded_call(tbk_model* m_, const double* d_k_, const double* h_k_, int64_t nk_)
    : m(m_), d_k(d_k_), h_k(h_k_), nk(nk_) {
    if (h_k == nullptr) return;
    f = tbk_fold_choose(m, h_k, nk, runs);
    if (f < 0) return;
    dim = m->dim;
    dim1 = dim - 1;
    nn2 = (size_t)m->n_orb * m->n_orb * 2;
    plan1 = &m->fold[f];
    for (int d = 0; d < dim; ++d)
        if (d != f) reduced.push_back(d);
}

int tbk_folded_call::begin() {
    TBK_CHECK(m->ws_kfold.reserve((size_t)nk * dim1 * sizeof(double)));
    d_k2 = m->ws_kfold.as<double>();
    return tbk_fold_drop_component(m, d_k, dim, f, nk, d_k2);
}

// The first-level operand of run r.  Runs are folded a group at a time (one pass over Bt for up to FOLD_GROUP of them): the
// group of r is folded if its operands are not in the plan's buffer.
int tbk_folded_call::run_operand(size_t r, tbk_operand_t* op) {
    if (group_lo < 0 || (int64_t)r < group_lo || (int64_t)r >= group_lo + FOLD_GROUP) {
        group_lo = (int64_t)r;
        const int n_g = (int)std::min<int64_t>(FOLD_GROUP, (int64_t)runs.size() - 1 - group_lo);
        double kf[FOLD_GROUP];
        for (int g = 0; g < n_g; ++g) kf[g] = h_k[runs[(size_t)(group_lo + g)] * dim + f];
        TBK_CHECK(tbk_fold_group(m, tbk_staged_operand(m), *plan1, kf, n_g, 0));
    }
    *op = plan1->operand((int)((int64_t)r - group_lo));
    return TBK_OK;
}

// [lo, hi) of one run with the operand `op` folded for that run: phase rows + contraction of the (dim - 1)-dimensional model
int tbk_folded_call::piece_plane(const tbk_operand_t& op, int64_t lo, int64_t hi, double* d_Hp) {
    const tbk_hk_plan_t plan = tbk_hk_plan(m, op, hi - lo, true);
    return chunk_h(m, plan, HK_TRI, 2, d_k2 + lo * dim1, nullptr, tbk_one_k_t(), d_Hp);
}

// lines a0, a0 + L, ... (n of them) of the first-level operand `from` -> slots slot0 ... of the second-level plan
// (the lines' shared-component values are read on the device: first point of every line)
int tbk_folded_call::fold_body(const tbk_operand_t& from, tbk_fold_plan_t& plan2, const LineInfo& li, int64_t a0, int64_t n, int slot0) {
    return tbk_fold_lines(m, from, plan2, d_k2 + a0 * dim1 + li.e2, li.L * dim1, (int)n, slot0);
}

// one launch for n lines whose operands are in slots 0 .. n - 1 (shared phase rows: the lines have equal coordinates)
int tbk_folded_call::contract_lines(tbk_fold_plan_t& plan2, const LineInfo& li, int64_t a0, int64_t n, double* d_Hp) {
    const tbk_operand_t op2 = plan2.operand(0);
    TBK_CHECK(m->ws_kline.reserve((size_t)li.L * std::max(dim1 - 1, 1) * sizeof(double)));
    TBK_CHECK(tbk_fold_drop_component(m, d_k2 + a0 * dim1, dim1, li.e2, li.L, m->ws_kline.as<double>()));
    TBK_CHECK(fill_rows(m, tbk_hk_plan(m, op2, li.L, true), m->ws_kline.as<double>()));  // (one k tile of rows)
    return tbk_launch_hk_dense_lines(m, op2, m->ws_phase.as<double>(), n, (int)li.L, plan2.k2 * plan2.row_len, d_Hp);
}

int tbk_folded_call::piece(const tbk_operand_t& op, int64_t lo, int64_t hi, double* d_Hp) {
    const LineInfo li = analyse(h_k, dim, reduced, lo, hi);
    if (!li.ok) return piece_plane(op, lo, hi, d_Hp);
    tbk_fold_plan_t* plan2 = nullptr;
    TBK_CHECK(tbk_fold_subplan(m, *plan1, li.e2, LINE_CAP, &plan2));
    if (!plan2 || plan2->n_rho * 3 > plan1->n_rho) return piece_plane(op, lo, hi, d_Hp);

    if (li.body > lo) TBK_CHECK(piece_plane(op, lo, li.body, d_Hp));  // ragged head
    for (int64_t l0 = 0; l0 < li.n_lines; l0 += LINE_CAP) {
        const int64_t nl = std::min<int64_t>(LINE_CAP, li.n_lines - l0);
        const int64_t a0 = li.body + l0 * li.L;
        TBK_CHECK(fold_body(op, *plan2, li, a0, nl, 0));
        TBK_CHECK(contract_lines(*plan2, li, a0, nl, d_Hp + (size_t)(a0 - lo) * nn2));
    }
    const int64_t body_end = li.body + li.n_lines * li.L;
    if (body_end < hi) TBK_CHECK(piece_plane(op, body_end, hi, d_Hp + (size_t)(body_end - lo) * nn2));  // ragged tail
    return TBK_OK;
}

// A chunk of WHOLE runs that are nothing but equal mesh lines (the planes of a mesh: run_schedule cuts chunks at
// run boundaries): the lines of all its planes are folded plane by plane into consecutive slots -- light launches
// that get through beside the previous chunk's reduction -- and contracted by ONE launch, instead of one contraction
// (which cannot start before the reduction has left the chip) and four light launches behind it per plane.
int tbk_folded_call::batched(int64_t c0, int64_t nkc, double* d_H, bool* done) {
    *done = false;
    const size_t r0 = (size_t)(std::upper_bound(runs.begin(), runs.end(), c0) - runs.begin()) - 1;
    if (runs[r0] != c0) return TBK_OK;
    size_t r1 = r0;
    while (r1 + 1 < runs.size() && runs[r1 + 1] <= c0 + nkc) ++r1;
    if (r1 - r0 < 2 || runs[r1] != c0 + nkc) return TBK_OK;  // fewer than two whole runs, or a cut run
    const LineInfo li0 = analyse(h_k, dim, reduced, runs[r0], runs[r0 + 1]);
    if (!li0.ok || li0.body != runs[r0] || li0.body + li0.n_lines * li0.L != runs[r0 + 1]) return TBK_OK;
    int64_t total = li0.n_lines;
    for (size_t r = r0 + 1; r < r1; ++r) {
        const LineInfo li = analyse(h_k, dim, reduced, runs[r], runs[r + 1]);
        if (!li.ok || li.e2 != li0.e2 || li.L != li0.L || li.body != runs[r] || li.body + li.n_lines * li.L != runs[r + 1] ||
            !same_line(h_k, dim, reduced, runs[r0], runs[r], li0.L, li0.e2))
            return TBK_OK;
        total += li.n_lines;
    }
    if (total > LINE_CAP) return TBK_OK;
    tbk_fold_plan_t* plan2 = nullptr;
    TBK_CHECK(tbk_fold_subplan(m, *plan1, li0.e2, LINE_CAP, &plan2));
    if (!plan2 || plan2->n_rho * 3 > plan1->n_rho) return TBK_OK;
    int slot = 0;
    for (size_t r = r0; r < r1; ++r) {
        tbk_operand_t op;
        TBK_CHECK(run_operand(r, &op));
        const int64_t n = (runs[r + 1] - runs[r]) / li0.L;
        TBK_CHECK(fold_body(op, *plan2, li0, runs[r], n, slot));
        slot += (int)n;
    }
    TBK_CHECK(contract_lines(*plan2, li0, c0, total, d_H));
    *done = true;
    return TBK_OK;
}

// Only the H(k) of a chunk is assembled run by run, each piece with the operand folded for its run.
int tbk_folded_call::build(int64_t c0, int64_t nkc, double* d_H) {
    {
        bool done = false;
        TBK_CHECK(batched(c0, nkc, d_H, &done));
        if (done) return TBK_OK;
    }
    size_t r = (size_t)(std::upper_bound(runs.begin(), runs.end(), c0) - runs.begin()) - 1;
    for (int64_t lo = c0; lo < c0 + nkc; ++r) {
        const int64_t hi = std::min(runs[r + 1], c0 + nkc);
        tbk_operand_t op;
        TBK_CHECK(run_operand(r, &op));
        TBK_CHECK(piece(op, lo, hi, d_H + (size_t)(lo - c0) * nn2));
        lo = hi;
    }
    return TBK_OK;
}
