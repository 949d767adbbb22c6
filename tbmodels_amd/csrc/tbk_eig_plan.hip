// tbk_eig_plan.hip -- which eigensolver kernels a call runs (host code only): the environment switches, tbk_eig_plan
// (tbk_internal.h) with the crossovers and their measurements, and what the entry points of tbk_api.hip do with a plan
// (tbk_eig_reserve, tbk_eig_reduce).  The kernel-shape tables stay with the kernels' launchers.

#include <algorithm>
#include <cstdlib>

#include "tbk_internal.h"

// the switches of DESIGN.md section 6, read once per process (the tests that set them start child processes)
const tbk_eig_env_t& tbk_eig_env() {
    static const tbk_eig_env_t env = [] {
        const auto num = [](const char* name, int unset) { const char* v = getenv(name); return v ? atoi(v) : unset; };
        return tbk_eig_env_t{num("TBK_BAND", 1) != 0,   num("TBK_BAND_SPLIT", 1) != 0, num("TBK_BAND_XL", 1) != 0, num("TBK_CHASE_WINDOW", 1) != 0,
                             num("TBK_REG128", 1) != 0, num("TBK_REG128_NW2", 1) != 0, num("TBK_BAND_XL_FROM", 1024)};
    }();
    return env;
}

// The two-stage kernels above 1024 orbitals: every panel as three launches with nothing per row in registers or LDS (band_xl_*).
// The limit is what has been validated (tests/test_gpu_parity.py: 1030 / 1536 / 2048 / 2050 / 3000 / 4096); nothing in the kernels
// depends on it.  TBK_BAND_XL=0: rocSOLVER above 1024 orbitals, as until round 4 (measurements).
static int band_maxn() { return tbk_eig_env().band_xl ? 4096 : BAND_ONE_WG_MAXN; }

bool tbk_eig_small_supported(int n) { return n >= 1 && n <= 64; }
// sizes the own solvers of tbk_eig_stream.hip and of tbk_eig_band.hip cover between them: the one-stage kernel up to 512
// orbitals, the two-stage reduction up to band_maxn() = 4096 (round 5: the launch chain of band_xl_* above 1024; with
// TBK_BAND_XL=0 the range ends at 1024 again); rocSOLVER above
bool tbk_eig_band_supported(int n) { return n > 64 && n <= band_maxn(); }

int tbk_eig_check_option(const tbk_model* m) {
    if (m->eigensolver == TBK_EIG_WAVE && !tbk_eig_small_supported(m->n_orb)) {
        tbk_set_error("TBK_EIG_WAVE handles n_orb <= 64 only (n_orb = %d)", m->n_orb);
        return TBK_ERR_ARGUMENT;
    }
    return TBK_OK;
}

// The two-stage kernels handle 64 < n <= 512 too; the two-stage path is TAKEN from 185 orbitals on (129 until round 3): up to 128 the one-stage kernel of
// tbk_eig_stream.hip (four waves per matrix, rows of two 64-column chunks) is faster -- 0.65 vs 0.84 us per matrix at 65
// orbitals, 1.73 vs 2.14 at 128; from 129 on the one-stage rows grow a third chunk and the order flips (3.8 vs 3.3 us at 160).
// (round 3: the one-stage kernel hands its last 128 steps to the register-resident kernels -- eight waves per matrix
// from 128 to 64, tbk_eig_small.hip -- which moved the crossover up: 1.34 vs 2.37 us per matrix at 130 orbitals, 1.96 vs
// 2.57 at 144, 2.56 vs 3.02 at 160; reduction stage of 4096 matrices 12.2 vs 12.7 ms at 176, 13.4 vs 13.9 at 184,
// 14.9 vs 14.4 at 192.  Round 4, after the trims of both stages, whole eigenval per k-point, one-stage vs two-stage:
// 2.85 vs 3.16 us at 168, 3.36 vs 3.34 at 176, 3.70 vs 3.70 at 184, 3.88 vs 3.78 at 188 -- 177 .. 192 orbitals pad to
// the same twelve blocks of 16, so the two-stage path takes over where the one-stage time reaches that: from 185)
constexpr int BAND_FROM = 185;

// Up to 768 orbitals the 16-slot window of the second stage: above 512 against the 32-slot window -- whole eigenval of 2048
// k-points 41.1 -> 39.1 us per k-point at 520 orbitals, 64.8 -> 62.9 at 640, 100.1 -> 97.4 at 768, 206.2 -> 215.6 at 1000.
constexpr int SMALL_WINDOW_MAXN = 768;

// Calls of at most max(4096, 768 n) k-points take the bisection kernel for every chunk: the lane-per-matrix QL
// is a serial chain of ~n^2 rotations (1.6 ms at n = 64 however few matrices there are) that only pays when tens of
// thousands of matrices share it and it can hide under the next chunk's reduction; bisection spends a wave per
// matrix (VALU work ~ n per matrix) and got ~1.7x faster with the secant steps of tbk_eig_stream.hip.  Measured
// crossover (ms per call, QL vs bisection): n = 64, N_R = 4096: 49152 k-points 57.29 vs
// 56.84, 57344: 66.71 vs 66.82, 100000: 114.4 vs 115.5; n = 48, N_R = 512: 30000: 5.94 vs 5.79, 40000: 7.55 vs 7.81;
// n = 32, N_R = 256: 16384: 1.45 vs 1.42, 24576: 1.84 vs 1.87.  (The rule was 640 n in round 1 and 384 n between the
// free-running QL and the faster bisection.)
constexpr int64_t TBK_SMALL_CALL = 4096;
constexpr int64_t TBK_SMALL_CALL_PER_ORBITAL = 768;
// (Up to 12 orbitals the QL chain used to be the shorter one -- 61 us at n = 8 -- until small matrices got the idle
// lanes of their wave for multisection: 1000 silicon k-points 59 -> 20 us, so small calls bisect at every size now.)

// Lanes per eigenvalue of the bisection kernel.  A few matrices cannot fill the chip with one lane per eigenvalue: spend lanes
// on shorter chains instead.  Small matrices get the lanes their first wave would leave idle anyway (8 orbitals: 8 per
// eigenvalue).
static int bisect_lanes(int n, int64_t call_nk) {
    int lpe = call_nk <= 32 ? 16 : call_nk <= 512 ? 4 : 1;
    if (n > 64) {
        // Above 64 orbitals (round 5): 16 or 4 lanes per eigenvalue at every size, over as many workgroups as that takes (until
        // round 4 the lanes had to fit ONE workgroup: 4 at 256 orbitals, 2 at 512 -- 31 sweeps where one lane with its secant steps
        // needs ~20 --, 1 above), while the call stays a few waves per CU: the sweeps are latency chains and idle lanes are free,
        // busy ones are not.  Measured (tools/bench_single_k.py, us of this stage, 1 / 4 / 16 lanes): one k-point at 256 orbitals
        // 188 / 160 / 114, at 512 414 / 370 / 244, at 1024 1348 / 1118 / 772; 64 k-points at 512 orbitals 462 / 404 / 800, at 1024
        // 1410 / 1300 / 3230, at 1536 1.8 / 3.5 ms / --.
        const int64_t eigenvalues = call_nk * (int64_t)n;
        if (lpe == 16 && eigenvalues * 16 > (int64_t(1) << 17)) lpe = 4;
        if (lpe == 4 && eigenvalues * 4 > (int64_t(1) << 18)) lpe = 1;
    } else {
        while (lpe < 16 && n * lpe * 2 <= 64) lpe *= 2;
        while (lpe > 1 && n * lpe > 1024) lpe /= 2;
    }
    return lpe;
}

tbk_eig_plan_t tbk_eig_plan(int n, int eigensolver, int64_t call_nk, int method) {
    const tbk_eig_env_t& env = tbk_eig_env();
    tbk_eig_plan_t p;
    p.n = n;
    p.call_nk = call_nk;
    // Own kernels or rocSOLVER, and the reduction family.  TBK_EIG_WAVE is the register-resident kernels alone (tbk_eig_check_option); the two-stage reduction unless TBK_BAND=0 asks
    // for the one-stage kernel; above 512 orbitals there is no one-stage kernel
    if (eigensolver == TBK_EIG_ROCSOLVER) return p;
    if (tbk_eig_small_supported(n))
        p.family = EIG_REGISTER;
    else if (eigensolver != TBK_EIG_AUTO || !tbk_eig_band_supported(n))
        return p;
    else if (method == TBK_REDUCE_TWO_STAGE)
        p.family = EIG_TWO_STAGE;
    else if (n > ST_MAXN)
        p.family = method == TBK_REDUCE_AUTO ? EIG_TWO_STAGE : EIG_ROCSOLVER;
    else
        p.family = (method == TBK_REDUCE_AUTO && env.band && n >= BAND_FROM) ? EIG_TWO_STAGE : EIG_ONE_STAGE;
    if (!p.own()) return p;
    // Register-resident kernels (the trailing 32 x 32 block as a second launch, tbk_eig_small.hip).  Calls of a few matrices (all of them resident at once: what counts is one matrix' latency, not
    // issue slots) keep the whole reduction in ONE launch of the four-wave kernel: a single 64 x 64 matrix 99 -> 78 us.  The
    // forms differ in the last bit.
    p.split_on = call_nk > 512;
    // One-stage: 65 .. 128 orbitals never leave the registers (round 3); above, the streaming kernel goes down to the trailing 128 x 128
    // block and the eight-wave register kernel to 64 x 64.  TBK_REG128=0 (measurements): the streaming kernel down to 64
    if (p.family == EIG_ONE_STAGE) {
        p.reg128 = env.reg128 && n <= 128;
        p.via128 = env.reg128 && n > 128;
        p.reg128_nw2 = env.reg128_nw2;
    }
    // Tridiagonal stage: up to 64 orbitals the lane-per-matrix QL unless the call is a small one (above); bisection above 64
    p.bisect = !tbk_eig_small_supported(n) || call_nk <= std::max<int64_t>(TBK_SMALL_CALL, TBK_SMALL_CALL_PER_ORBITAL * (int64_t)n);
    p.bisect_lanes = bisect_lanes(n, call_nk);
    if (p.family != EIG_TWO_STAGE) return p;

    // Two-stage, first stage.  The sizes that take the launch chain of band_xl_* whatever the call: above 1024 orbitals (TBK_BAND_XL_FROM=n: above n -- tests
    // run the chain at sizes the NumPy model is quick at, and A/B it against the one-workgroup kernels)
    p.chain_by_size = n > env.band_xl_from;
    // Calls of a few matrices (Z2Pack-style lines and single k-points, _tb_model.py:1103-1108; band-structure paths of a few dozen
    // points): the first stage as a chain of launches, so that every tile pass runs on several CUs per matrix instead of one
    // (never fused with stage two; the partial sums differ from one workgroup's in the last bit).  TBK_BAND_SPLIT=0: off (an
    // independent reference path for the tests).
    // as long as every member workgroup of every matrix finds a CU of its own: n_cu / members matrices (on 256 CUs: 64 up to
    // 512 orbitals, 32 at 1024).  Measured (one k-point per call, reduction stage): 256 orbitals 2.11 -> 2.04 ms, 384: 4.62 -> 3.80, 512: 8.31 ->
    // 6.01, 1024: 49.0 -> 24.4
    // (up to 256 orbitals the serial launches dominate and 64 matrices in one launch are as fast: 2.49 vs 2.40 ms -- 8 there)
    // Round 5: the chain these calls take is the one of band_xl_* (three launches per panel, sweeps on a workgroup per block row =
    // every CU for ONE matrix; round 4's chain had two launches per panel and 4 - 8 member workgroups per matrix).  One-k
    // eigenval, round-4 chain -> band_xl chain: 2.05 -> 1.94 ms at 256 orbitals, 3.99 -> 3.50 at 384, 6.05 -> 5.03 at 512, 13.98
    // -> 10.28 at 768, 24.35 -> 16.84 at 1024; 64 matrices: 2.23 -> 2.31 / 4.39 -> 4.43 / 6.80 -> 7.16 / 22.5 -> 17.6 / 46.3 ->
    // 35.1; 64 matrices of 512 orbitals in ONE launch of the eight-wave kernel: 8.09 ms -- so calls of up to 8 matrices up to 256
    // orbitals, 64 up to 512, 96 above.
    const bool few = env.band_split && n > 128 && n <= BAND_ONE_WG_MAXN && call_nk <= (n <= 256 ? 8 : n <= 512 ? 64 : 96);
    p.chain = p.chain_by_size || few;
    // One workgroup per matrix, calls of a few matrices (one k-point per call is what Z2Pack-style callers do, _tb_model.py:1103-1108):
    // every matrix has a CU to itself anyway, so it gets EIGHT waves and one row per thread.  The partial sums of eight waves
    // differ from those of four in the last bit.
    p.wide = n <= 512 && call_nk <= 128;
    // Second stage.  Both stages in ONE kernel (the workgroup goes straight on to the bulge chasing of its matrix, in the same LDS) or in
    // two launches with the second one on the tridiagonal stream next to the following chunk's first stage.  Per matrix
    // the two cost the same -- a workgroup's critical path is the sum of its phases either way -- and in the chunk pipeline
    // fused is 1 % ahead at 256 orbitals (cfg3 134.1 vs 132.3 k k-points/s), 4 % behind at 512 (cfg5 13.5 vs 14.0 k: one
    // workgroup per CU there, and the separate launch fills the gaps of the next chunk's first stage).
    // (the launch chain ends in the band's way out; the second stage is a launch of its own)
    p.fused = n <= 256 && !p.chain;
    // 257 - 768 orbitals, calls of more matrices than the chip has CUs: the windowed kernel with 16 sweep slots and 272 columns -- 78 KiB
    // of LDS instead of the 133 KiB of the plain LDS form at 512 orbitals, so two of its workgroups share a CU, or one sits beside a
    // first-stage workgroup of the next chunk (76 KiB).  A matrix takes more and slower ticks (1293 x ~2.2 us instead of 1088 x 1.55 at
    // 512 orbitals), the chip holds twice as many: cfg5 16.04 -> 16.63 k k-points/s, whole eigenval of 2048 k-points 12.93 -> 11.74 us per
    // k-point at 320 orbitals, 18.82 -> 17.66 at 384, 34.57 -> 33.64 at 512; the same bits.
    // Above 512 orbitals the 32-slot window in front of the diagonals in global memory (tbk_eig_band_chase.hip).
    // TBK_CHASE_WINDOW=0 (measurements): no windowed kernel -- above 512 orbitals the global-memory form, the plain LDS form below
    const bool small_window = env.chase_window && n > 256 && n <= SMALL_WINDOW_MAXN && call_nk > 256;
    if (small_window)
        p.chase = EIG_CHASE_WINDOW16;
    else if (n > BAND_LDS_CHASE_MAXN)
        p.chase = env.chase_window ? EIG_CHASE_WINDOW32 : EIG_CHASE_GLOBAL;
#ifdef TBK_ABLATE_WIN_FORCE  // (timing: the 32-slot window from 257 orbitals on, at every call size)
    if (n > 256) p.chase = env.chase_window ? EIG_CHASE_WINDOW32 : EIG_CHASE_GLOBAL;
#endif
    // does a matrix' band buffer carry the 16 working diagonals behind the compact band: by the size alone (any call of a size
    // above 256 orbitals may need them), so that a buffer's stride does not depend on the call
    p.chase_buffer = n > 256;
    p.band_stride = tbk_band_bytes_per_matrix(n, p.chase_buffer);
    p.ws_band = tbk_band_scratch_per_matrix(n);
    p.ws_bandmat = p.fused ? 0 : p.band_stride;
    p.ws_xl = p.chain ? (size_t)n * n * 2 * sizeof(double) : 0;  // the second matrix buffer of the chain
    return p;
}

// (tbk_band_launch_xl; by the matrices of the LAUNCH: per matrix the same launches in the same order, the same bits)
int tbk_eig_xl_groups(const tbk_eig_plan_t& plan, int64_t nk) {
    constexpr int XL_GROUPS = 2;  // (1 - 4 were measured)
    return (plan.chain_by_size && nk >= 4 * XL_GROUPS) ? XL_GROUPS : 1;
}

// What the chunk length is sized with (choose_chunk, tbk_api.hip): (d, e) + complex tau, and an upper bound over the plans a
// size in the two-stage kernels' range can get -- the scratch and both band buffers also where a call takes the one-stage
// path or the fused kernel, the chain's second matrix buffer only where every call takes the chain.
size_t tbk_eig_scratch_per_k(const tbk_model* m) {
    const int n = m->n_orb;
    const size_t de = (size_t)n * 4 * sizeof(double) + sizeof(int);
    if (!tbk_eig_band_supported(n)) return de;
    const tbk_eig_plan_t batch = tbk_eig_plan(n, TBK_EIG_AUTO, int64_t(1) << 40, TBK_REDUCE_TWO_STAGE);  // (a call too long for the few-matrices chain)
    return de + batch.ws_band + 2 * batch.band_stride + batch.ws_xl;
}

int tbk_eig_reserve(tbk_model* m, const tbk_eig_plan_t& plan, int64_t max_nk, int bandmats) {
    TBK_CHECK(m->ws_band.reserve((size_t)max_nk * plan.ws_band));
    for (int b = 0; b < bandmats; ++b) TBK_CHECK(m->ws_bandmat[b].reserve((size_t)max_nk * plan.ws_bandmat));
    return m->ws_xl.reserve((size_t)max_nk * plan.ws_xl);
}

int tbk_eig_reduce(tbk_model* m, const tbk_eig_plan_t& plan, hipStream_t s, double* d_H, int64_t nk, double* d_de, void* d_band) {
    switch (plan.family) {
        case EIG_REGISTER: return tbk_launch_tridiag(m, plan, s, d_H, nk, d_de);
        case EIG_ONE_STAGE: return tbk_launch_tridiag_stream(m, plan, s, d_H, nk, d_de);
        case EIG_TWO_STAGE: break;
        default: tbk_set_error("no reduction kernel for n_orb = %d with this method", plan.n); return TBK_ERR_ARGUMENT;
    }
    if (d_band) return tbk_launch_band_reduce(m, plan, s, d_H, nk, m->ws_band.ptr, d_band);
    if (plan.fused) return tbk_launch_band_reduce(m, plan, s, d_H, nk, m->ws_band.ptr, nullptr, d_de);
    // (a batch in groups: the second stage of every group behind its first stage, on the group's stream)
    if (tbk_eig_xl_groups(plan, nk) > 1) return tbk_launch_band_reduce(m, plan, s, d_H, nk, m->ws_band.ptr, m->ws_bandmat[0].ptr, d_de);
    TBK_CHECK(tbk_launch_band_reduce(m, plan, s, d_H, nk, m->ws_band.ptr, m->ws_bandmat[0].ptr));
    return tbk_launch_band_chase(m, plan, s, m->ws_bandmat[0].ptr, nk, d_de);
}
