// The mean-variance arithmetic of main.py:243-286 as device functions, shared by mv_select_kernel (sampler.hip: one lane per
// candidate of a training interaction) and recommend_mv_topk_kernel (recommend.hip: the whole candidate list of a user).
// fp64 in numpy's order of operations and WITHOUT contraction: every product is rounded before it is added, as numpy's are, and
// both kernels get the same instructions whatever the translation unit's default is.
#pragma once
#include "common.hpp"

// y_mv of the candidate whose returns are row `stock` of `day` (f64[n_stocks, n_ret]) against the portfolio port[0:plen].
// CHECK: entries of `port` outside [0, n_stocks) are left out and do not count as holdings (the serving kernel takes portfolios
// from a caller); without it every entry is taken as it is (the training path packs its own).  No holding: main.py:254.
// (np.mean's summation order: pfo_np_sum; np.cov: deviations from the mean, products summed in index order, c *= 1/(N - 1);
// np.sum over fewer than eight covariances is sequential.)
template <bool CHECK>
__device__ __forceinline__ double pfo_mv_value(const double* __restrict__ day, int stock, int n_stocks, int n_ret,
                                               const int32_t* __restrict__ port, int plen, double gamma) {
#pragma clang fp contract(off)
  const double* ri = day + (int64_t)stock * n_ret;
  const double mu = pfo_np_sum(ri, n_ret) / (double)n_ret;                  // main.py:243
  const double inv = 1.0 / (double)(n_ret - 1);                         // np.cov: c *= 1/(N - ddof)
  double var = 0.0;
  for (int t = 0; t < n_ret; ++t) var += (ri[t] - mu) * (ri[t] - mu);
  var *= inv;
  int n_hold = 0;
  double ssum = 0.0;
  for (int p = 0; p < plen; ++p) {
    const int s = port[p];
    if (CHECK && (unsigned)s >= (unsigned)n_stocks) continue;
    ++n_hold;
    const double* rp = day + (int64_t)s * n_ret;
    const double mp = pfo_np_sum(rp, n_ret) / (double)n_ret;
    double cv = 0.0;
    for (int t = 0; t < n_ret; ++t) cv += (ri[t] - mu) * (rp[t] - mp);
    ssum += cv * inv;                                                   // np.sum(sigma_ij), main.py:268
  }
  if (n_hold == 0) return (mu / gamma) / var;                           // main.py:254
  const double sum_sigma = (1.0 / (double)n_hold) * ssum;               // y_uj/n_holding * sum
  return (mu / gamma - 0.5 * sum_sigma) / var;                          // main.py:271
}

// scipy.stats.rankdata's average-tie rank of a value with `less` smaller and `eq` equal values (itself among them), main.py:282
__device__ __forceinline__ double pfo_mv_avg_rank(int less, int eq) {
#pragma clang fp contract(off)
  return (double)less + ((double)eq + 1.0) * 0.5;
}

// main.py:286
__device__ __forceinline__ double pfo_mv_blend(double invest, double tgn, double lam) {
#pragma clang fp contract(off)
  return invest * lam + tgn * (1.0 - lam);
}
