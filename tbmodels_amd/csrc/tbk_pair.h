// tbk_pair.h -- what the kernels that weigh pairs of band states at one chemical potential and one temperature share: tbk_chi.hip (the
// susceptibilities) and tbk_optics.hip (the optical conductivity).  The two Fermi tables f, 1 - f of a list of eigenvalues, the
// cancellation-free pair factors made from them, and the fixed wave sum.  DESIGN.md 15.2 has the derivation.
#pragma once

#include "tbk_internal.h"

#include <cmath>

constexpr int PAIR_THREADS = 256;

// the frequencies omega[n_w] and the broadening of a dynamic call (too_many: the family's text for n_w > most)
inline int pair_check_frequencies(int64_t n_w, int64_t most, const double* omega, double eta, const char* too_many) {
    TBK_ARG(n_w >= 1, "n_w < 1");
    TBK_ARG(n_w <= most, too_many);
    TBK_ARG(omega != nullptr, "omega is NULL");
    for (int64_t j = 0; j < n_w; ++j) TBK_ARG(std::isfinite(omega[j]), "a frequency is not finite");
    TBK_ARG(std::isfinite(eta) && eta > 0.0 && eta * eta > 0.0, "eta is not finite or not positive (or its square underflows)");
    return TBK_OK;
}

// f(lo) (1 - f(hi)) h((lo - hi) / T) >= 0 of one pair of states: -T F
static __device__ __forceinline__ double chi_pair_weight(double ea, double fa, double ga, double eb, double fb, double gb, double inv_t) {
    const bool a_low = ea <= eb;
    const double lo = a_low ? ea : eb, hi = a_low ? eb : ea;
    const double y = (lo - hi) * inv_t;
    const double h = y < 0.0 ? expm1(y) / y : 1.0;  // (-inf: 0)
    return (a_low ? fa : fb) * (a_low ? gb : ga) * h;
}

// g = f(a) - f(b) of one pair of states, |g| <= 1: +-f(lo) (1 - f(hi)) (-expm1((lo - hi) / T)), + where a <= b; a zero for a == b
static __device__ __forceinline__ double chi_pair_difference(double ea, double fa, double ga, double eb, double fb, double gb, double inv_t) {
    const bool a_low = ea <= eb;
    const double lo = a_low ? ea : eb, hi = a_low ? eb : ea;
    const double v = (a_low ? fa : fb) * (a_low ? gb : ga) * (-expm1((lo - hi) * inv_t));
    return a_low ? v : -v;
}

// all 64 lanes, the same tree whatever the values
static __device__ __forceinline__ double chi_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// f and 1 - f of one state from ONE exponential, t = exp(-|E - mu| / T): (t, 1) / (1 + t) above mu, (1, t) / (1 + t) at and below
// it -- 1 - f(x) = f(2 mu - x) at the mirrored distance, which is -(E - mu) without a rounding
static __global__ void __launch_bounds__(PAIR_THREADS) chi_fermi_kernel(const double* __restrict__ E, int64_t items, double mu, double T,
                                                                double* __restrict__ tab) {
    const int64_t i = (int64_t)blockIdx.x * PAIR_THREADS + threadIdx.x;
    if (i >= items) return;
    const double d = E[i] - mu;
    const double t = exp(-fabs(d) / T);
    const double small = t / (1.0 + t), big = 1.0 / (1.0 + t);
    tab[i] = d > 0.0 ? small : big;
    tab[items + i] = d < 0.0 ? small : big;
}
