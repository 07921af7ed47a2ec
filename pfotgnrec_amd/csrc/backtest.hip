// A served list scored against what happened (include/pfotgn.h, pfo_list_metrics): the place of the item the user then took
// in the list, recall / NDCG at up to eight cutoffs, and the change of annualised return and Sharpe ratio when the first c
// stocks of the list join the user's portfolio - in-sample and out-of-sample, each table with its own day index.
//
// The investment stage is eval.hip's (eval_daily_sums / eval_return_sharpe) generalised from "1, 3, 5" to the cutoffs: the same
// fp64 operations in the same order, no contraction, so at cutoffs (1, 3, 5) on the list pfo_eval_metrics wrote to top5_item
// the twelve values are its invest_out to the bit.  The operations are written down again here rather than shared: eval.hip's
// kernels keep their code, registers and bits.
//
// One wavefront (a 64-lane workgroup) per user.
//   R  lane t < L holds slot t of the list; the rank is the first set bit of one ballot.  Lanes c < n_c write hits / NDCG.
//   B  per table, lanes r < n_ret (two passes beyond 64) hold column r of the per-day log-return sums: the portfolio rows first,
//      the list's slots added one by one, divided by the row count behind the portfolio and at every cutoff -> daily[2][1 + n_c][n_ret]
//   C  2 (1 + n_c) lanes, one per daily series: mean and population deviation in numpy's summation order (pfo_np_sum).
//   D  4 n_c lanes write new - old.
// LDS: 2 (1 + n_c) (n_ret + 2) doubles + 72 ints: 19.0 KB at n_c = 8, n_ret = 128.  No atomics, nothing but vector stores.
#include "common.hpp"

#pragma clang fp contract(off)

#define PFO_LIST_MAX_L 64
#define PFO_LIST_MAX_CUT 8
#define PFO_LIST_MAX_RET 128

namespace {

struct ListCuts {
  int n;
  int c[PFO_LIST_MAX_CUT];
};

struct ListTable {
  const double* ret;
  const int32_t* day;
  int n_days, n_stocks;
};

__global__ __launch_bounds__(64) void list_metrics_kernel(
    const int32_t* __restrict__ list_item, const int32_t* __restrict__ n_valid, const int32_t* __restrict__ truth, int L,
    const ListCuts cuts, const int32_t* __restrict__ port_idx, const int32_t* __restrict__ port_len, int port_stride, int upper_u,
    const ListTable past, const ListTable future, int n_ret, int64_t out_row0, int32_t* __restrict__ rank_out,
    float* __restrict__ hits, float* __restrict__ ndcg, double* __restrict__ invest) {
  extern __shared__ double lds_list[];
  const int n_c = cuts.n, S = 1 + n_c;                           // S series per table: the portfolio alone, then one per cutoff
  double* daily = lds_list;                                      // [2][S][n_ret]
  double* res = daily + 2 * S * n_ret;                           // [2][S][2]: return, sharpe
  int* item = reinterpret_cast<int*>(res + 4 * S);               // [64]: the list, -1 = nothing in this slot
  int* cut = item + 64;                                          // [8]: the cutoffs (read with a running index below)
  const int64_t b = blockIdx.x, o = out_row0 + b;
  const int lane = threadIdx.x;

  // ---- R: the list and the truth's place in it
  int nv = n_valid ? n_valid[b] : L;
  nv = min(max(nv, 0), L);
  const int want = truth[b];
  const int it = (lane < nv) ? list_item[b * L + lane] : -1;     // (nv <= L: slots behind the list are never read)
  item[lane] = it < 0 ? -1 : it;
  const unsigned long long found = __ballot(want >= 0 && it >= 0 && it == want);
  const int rank = found ? (int)__builtin_ctzll(found) : PFO_EVAL_RANK_NONE;
  if (lane == 0 && rank_out) rank_out[o] = rank;
  int my_cut = cuts.c[0];                                        // lane i < 8: cutoff i (0 behind the last)
#pragma unroll
  for (int i = 1; i < PFO_LIST_MAX_CUT; ++i) my_cut = lane == i ? cuts.c[i] : my_cut;
  if (lane < PFO_LIST_MAX_CUT) cut[lane] = my_cut;
  if (lane < n_c) {
    const bool hit = rank < my_cut;
    if (hits) hits[o * n_c + lane] = hit ? 1.f : 0.f;
    // idcg = 1; the expression of eval_write_ranking, so that the two kernels agree to the bit at every rank both can state
    if (ndcg) ndcg[o * n_c + lane] = hit ? 1.f / log2f((float)rank + 2.f) : 0.f;
  }
  __syncthreads();

  // ---- B: a day or a stock outside a table poisons THAT table's sums instead of reading out of bounds
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  const int plen = port_stride > 0 ? min(max(port_len[b], 0), port_stride) : 0;
  const int depth = cut[n_c - 1];                                // <= L: no slot behind the last cutoff matters
  for (int tbl = 0; tbl < 2; ++tbl) {
    const ListTable& T = tbl == 0 ? past : future;
    const int day = T.day[b];
    const bool day_ok = day >= 0 && day < T.n_days;
    const double* base = T.ret + (int64_t)(day_ok ? day : 0) * T.n_stocks * n_ret;
    for (int r = lane; r < n_ret; r += 64) {
      double s = 0.0;
      int cnt = 0;
      for (int p = 0; p < plen; ++p) {
        const int st = port_idx[b * port_stride + p];
        s += (day_ok && st >= 0 && st < T.n_stocks) ? base[(int64_t)st * n_ret + r] : nan;
        ++cnt;
      }
      daily[(tbl * S) * n_ret + r] = s / (double)cnt;            // (unused when the portfolio is empty)
      int ci = 0;
      for (int t = 0; t < depth; ++t) {
        const int id = item[t];
        if (id >= 0) {
          const int64_t st = (int64_t)id - upper_u - 1;
          s += (day_ok && st >= 0 && st < T.n_stocks) ? base[st * n_ret + r] : nan;
          ++cnt;
        }
        if (ci < n_c && t + 1 == cut[ci]) {
          daily[(tbl * S + 1 + ci) * n_ret + r] = s / (double)cnt;
          ++ci;
        }
      }
    }
  }
  __syncthreads();

  // ---- C: return and Sharpe ratio of each series
  if (lane < 2 * S) {
    double ret = 0.0, sharpe = 0.0;                              // an empty portfolio alone: 0, 0
    if ((lane % S) != 0 || plen > 0) {
      double* x = daily + lane * n_ret;
      const double mean = pfo_np_sum(x, n_ret) / (double)n_ret;
      for (int i = 0; i < n_ret; ++i) {
        const double d = x[i] - mean;
        x[i] = d * d;
      }
      const double sd = sqrt(pfo_np_sum(x, n_ret) / (double)n_ret);
      ret = mean * 251.0;
      sharpe = ret / (sd * 15.84297951775486);                   // np.sqrt(251)
    }
    res[2 * lane] = ret;
    res[2 * lane + 1] = sharpe;
  }
  __syncthreads();

  // ---- D: (return@c.. | sharpe@c..) x (in-sample | out-of-sample)
  if (lane < 4 * n_c && invest) {
    const int tbl = lane / (2 * n_c), kind = (lane % (2 * n_c)) / n_c, ci = lane % n_c;
    invest[o * (4 * n_c) + lane] = res[2 * (tbl * S + 1 + ci) + kind] - res[2 * (tbl * S) + kind];
  }
}

}  // namespace

extern "C" int pfo_list_metrics(const int32_t* list_item, const int32_t* n_valid, const int32_t* truth, int64_t U, int32_t L,
                                const int32_t* cutoffs, int32_t n_c, const int32_t* port_idx, const int32_t* port_len,
                                int32_t port_stride, int32_t upper_u, const double* ret_past, const int32_t* day_past,
                                int32_t past_days, int32_t past_stocks, const double* ret_future, const int32_t* day_future,
                                int32_t future_days, int32_t future_stocks, int32_t n_ret, int64_t out_row0, int64_t out_rows,
                                int32_t* rank_out, float* hits_out, float* ndcg_out, double* invest_out, void* stream) {
  PFO_REQUIRE(U >= 0 && U <= 2147483647, "U must be in [0, 2^31)");
  PFO_REQUIRE(L >= 1 && L <= PFO_LIST_MAX_L, "L must be in [1, 64]");
  PFO_REQUIRE(n_c >= 1 && n_c <= PFO_LIST_MAX_CUT, "n_c must be in [1, 8]");
  PFO_REQUIRE(n_ret >= 2 && n_ret <= PFO_LIST_MAX_RET, "n_ret must be in [2, 128]");
  PFO_REQUIRE(past_days > 0 && past_stocks > 0 && future_days > 0 && future_stocks > 0 && port_stride >= 0, "bad table sizes");
  PFO_REQUIRE(out_row0 >= 0 && out_rows >= 0 && out_row0 <= out_rows - U, "rows [out_row0, out_row0 + U) exceed the output buffers");
  PFO_REQUIRE(cutoffs, "null cutoffs");                          // (a host array: the one pointer the bounds are read through)
  ListCuts cuts;
  cuts.n = n_c;
  for (int i = 0; i < PFO_LIST_MAX_CUT; ++i) cuts.c[i] = i < n_c ? cutoffs[i] : 0;
  for (int i = 0; i < n_c; ++i)
    PFO_REQUIRE(cuts.c[i] >= 1 && cuts.c[i] <= L && (i == 0 || cuts.c[i] > cuts.c[i - 1]),
                "cutoffs must be strictly increasing and lie in [1, L]");
  if (U == 0) return PFO_OK;
  PFO_REQUIRE(list_item && truth && ret_past && day_past && ret_future && day_future, "null input");
  PFO_REQUIRE((port_idx && port_len) || port_stride == 0, "null port_idx / port_len");
  const int S = 1 + n_c;
  const size_t shmem = (size_t)(2 * S * n_ret + 4 * S) * sizeof(double) + (64 + PFO_LIST_MAX_CUT) * sizeof(int);
  const ListTable past = {ret_past, day_past, (int)past_days, (int)past_stocks};
  const ListTable future = {ret_future, day_future, (int)future_days, (int)future_stocks};
  hipStream_t s = (hipStream_t)stream;
  PFO_KLAUNCH(list_metrics_kernel, dim3((unsigned)U), dim3(64), shmem, s, list_item, n_valid, truth, (int)L, cuts, port_idx, port_len,
              (int)port_stride, (int)upper_u, past, future, (int)n_ret, out_row0, rank_out, hits_out, ndcg_out, invest_out);
  PFO_LAUNCH_CHECK();
  return PFO_OK;
}
