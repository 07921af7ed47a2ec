// The mean-variance arithmetic of main.py:243-286 as device functions, shared by mv_select_kernel (sampler.hip: one lane per
// candidate of a training interaction), recommend_mv_topk_kernel (recommend.hip: the whole candidate list of a user) and
// recommend_basket_topk_kernel (recommend.hip: the same list, re-ranked after every pick).
// fp64 in numpy's order of operations and WITHOUT contraction: every product is rounded before it is added, as numpy's are, and
// both kernels get the same instructions whatever the translation unit's default is.
#pragma once
#include "common.hpp"

// The pieces of y_mv.  pfo_mv_value below is their composition over a whole portfolio; recommend_basket_topk_kernel keeps mu, var
// and the running sum per candidate and takes one pfo_mv_add_cov step per pick - the same rounded operations in the same order.
// (np.mean's summation order: pfo_np_sum; np.cov: deviations from the mean, products summed in index order, c *= 1/(N - 1);
// np.sum over fewer than eight covariances is sequential.)
__device__ __forceinline__ double pfo_mv_mean(const double* r, int n_ret) {
#pragma clang fp contract(off)
  return pfo_np_sum(r, n_ret) / (double)n_ret;                          // main.py:243
}

__device__ __forceinline__ double pfo_mv_inv(int n_ret) {
#pragma clang fp contract(off)
  return 1.0 / (double)(n_ret - 1);                                     // np.cov: c *= 1/(N - ddof)
}

// variance of the row ri with mean mu
__device__ __forceinline__ double pfo_mv_var(const double* ri, double mu, int n_ret, double inv) {
#pragma clang fp contract(off)
  double var = 0.0;
  for (int t = 0; t < n_ret; ++t) var += (ri[t] - mu) * (ri[t] - mu);
  var *= inv;
  return var;
}

// ssum + cov(ri, rp): one more holding (row rp, mean mp) in np.sum(sigma_ij), main.py:268
__device__ __forceinline__ double pfo_mv_add_cov(double ssum, const double* ri, double mu,
                                                 const double* rp, double mp, int n_ret, double inv) {
#pragma clang fp contract(off)
  double cv = 0.0;
  for (int t = 0; t < n_ret; ++t) cv += (ri[t] - mu) * (rp[t] - mp);
  return ssum + cv * inv;
}

// y_mv from the pieces; ssum: the sum over the n_hold holdings
__device__ __forceinline__ double pfo_mv_finish(double mu, double gamma, double var, double ssum, int n_hold) {
#pragma clang fp contract(off)
  if (n_hold == 0) return (mu / gamma) / var;                           // main.py:254
  const double sum_sigma = (1.0 / (double)n_hold) * ssum;               // y_uj/n_holding * sum
  return (mu / gamma - 0.5 * sum_sigma) / var;                          // main.py:271
}

// y_mv of the candidate whose returns are row `stock` of `day` (f64[n_stocks, n_ret]) against the portfolio port[0:plen].
// CHECK: entries of `port` outside [0, n_stocks) are left out and do not count as holdings (the serving kernel takes portfolios
// from a caller); without it every entry is taken as it is (the training path packs its own).  No holding: main.py:254.
template <bool CHECK>
__device__ __forceinline__ double pfo_mv_value(const double* __restrict__ day, int stock, int n_stocks, int n_ret,
                                               const int32_t* __restrict__ port, int plen, double gamma) {
  const double* ri = day + (int64_t)stock * n_ret;
  const double mu = pfo_mv_mean(ri, n_ret);
  const double inv = pfo_mv_inv(n_ret);
  const double var = pfo_mv_var(ri, mu, n_ret, inv);
  int n_hold = 0;
  double ssum = 0.0;
  for (int p = 0; p < plen; ++p) {
    const int s = port[p];
    if (CHECK && (unsigned)s >= (unsigned)n_stocks) continue;
    ++n_hold;
    const double* rp = day + (int64_t)s * n_ret;
    ssum = pfo_mv_add_cov(ssum, ri, mu, rp, pfo_mv_mean(rp, n_ret), n_ret, inv);
  }
  return pfo_mv_finish(mu, gamma, var, ssum, n_hold);
}

// ---- the position-weighted form: holding p weighs pw[p] in place of 1 / n_hold.
// A weight counts iff it is finite and > 0 (a NaN compares false both times).
__device__ __forceinline__ bool pfo_mv_weight_counts(double w) { return w > 0.0 && w <= 1.79769313486231570815e308; }

// ssum + w * cov(ri, rp): the covariance as in pfo_mv_add_cov, then one rounded product, then one rounded add.  w == 1.0 is
// pfo_mv_add_cov to the bit.
__device__ __forceinline__ double pfo_mv_add_wcov(double ssum, double w, const double* ri, double mu, const double* rp, double mp,
                                                  int n_ret, double inv) {
#pragma clang fp contract(off)
  double cv = 0.0;
  for (int t = 0; t < n_ret; ++t) cv += (ri[t] - mu) * (rp[t] - mp);
  const double wc = w * (cv * inv);
  return ssum + wc;
}

// y_mv from the pieces; ssum_w: the weighted sum over the n_hold counted holdings, wsum: the sum of their weights (all ones:
// wsum == n_hold exactly, and this is pfo_mv_finish to the bit)
__device__ __forceinline__ double pfo_mv_finish_weighted(double mu, double gamma, double var, double ssum_w, double wsum, int n_hold) {
#pragma clang fp contract(off)
  if (n_hold == 0) return (mu / gamma) / var;                           // main.py:254
  const double sum_sigma = (1.0 / wsum) * ssum_w;
  return (mu / gamma - 0.5 * sum_sigma) / var;                          // main.py:271
}

// pfo_mv_value<true> with the weight row pw[0:plen] beside port[0:plen]: a holding counts iff its stock is in [0, n_stocks) and
// its weight counts; wsum is the sequential sum of the counted weights in row order.
__device__ __forceinline__ double pfo_mv_value_weighted(const double* __restrict__ day, int stock, int n_stocks, int n_ret,
                                                        const int32_t* __restrict__ port, const double* __restrict__ pw, int plen,
                                                        double gamma) {
#pragma clang fp contract(off)
  const double* ri = day + (int64_t)stock * n_ret;
  const double mu = pfo_mv_mean(ri, n_ret);
  const double inv = pfo_mv_inv(n_ret);
  const double var = pfo_mv_var(ri, mu, n_ret, inv);
  int n_hold = 0;
  double ssum = 0.0, wsum = 0.0;
  for (int p = 0; p < plen; ++p) {
    const int s = port[p];
    const double w = pw[p];
    if ((unsigned)s >= (unsigned)n_stocks || !pfo_mv_weight_counts(w)) continue;
    ++n_hold;
    wsum += w;
    const double* rp = day + (int64_t)s * n_ret;
    ssum = pfo_mv_add_wcov(ssum, w, ri, mu, rp, pfo_mv_mean(rp, n_ret), n_ret, inv);
  }
  return pfo_mv_finish_weighted(mu, gamma, var, ssum, wsum, n_hold);
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
