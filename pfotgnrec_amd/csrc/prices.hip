// Price ledger (PriceLedger): the log-return table of the mean-variance rank, returns f64[day_cap, stock_cap, n_ret],
// grown by one trading day per call, and the trading day of a timestamp found on the device.
//
// Layout.  The day axis is a ring of day_cap slots; a day's block is stock_cap rows of n_ret doubles, so the query kernels
// (pfo_mv_select, pfo_recommend_mv_topk, pfo_recommend_basket_topk) read `returns + slot * stock_cap * n_ret` unchanged when
// they are given day_cap as n_days and stock_cap as n_stocks.  Row s of day d is the window of the n_ret newest log-returns of
// stock s as of day d, oldest first.  A row nobody ever quoted is all zeros, and so is every row behind the live stock count:
// by the NaN rule of mv_value.hpp a constant series has y = 0/0, so such a stock sits out of every order until its window holds
// two different closes.
//
// Append.  The window of day d is the window of day d - 1 shifted by one, so one lane per ELEMENT of the new day's live block:
//   j < n_ret - 1 : R[new, s, j] = R[prev, s, j + 1], copied as 64-bit words (no arithmetic touches them);
//   j = n_ret - 1 : quoted and last_close[s] not NaN -> log(close / last_close[s]), the IEEE quotient, then log; else +0;
//                   last_close[s] = close where quoted (this lane is the only reader and writer of last_close[s]).
// Consecutive lanes sit on consecutive addresses of the new row; the shifted read is the same row of the previous slot, one
// element on.  16 B of traffic per element, no atomics, no lane waits for another.  prev_slot != new_slot is required: the
// copy is not in place.
//
// Sparse closes.  (stocks i32[m], closes f64[m]) become the dense form through the stamp scheme of holdings.hip: a cleared
// stamp table i32[n_stocks], atomicMax(stamp[s], p + 1) over the VALID positions (index inside the table, close positive and
// finite), and the append launch reads closes[stamp[s] - 1].  Integer maxima commute: among repeated indices the last valid
// position wins whatever the launch geometry.
//
// Lookup.  key = (int64) floor(ts / key_divisor), binary search over the strictly increasing keys of the live days in ring order.
//
// Every index that comes from device memory is range-checked before it addresses anything.
#include "common.hpp"
#include <algorithm>
#include <cmath>

namespace {

constexpr int PRICE_BLOCK = 256;
constexpr int64_t PRICE_MAX_GRID = 1 << 20;       // beyond that the lanes stride

unsigned price_grid(int64_t total) { return (unsigned)std::min<int64_t>(pfo_ceil_div(total, PRICE_BLOCK), PRICE_MAX_GRID); }

__device__ __forceinline__ bool close_ok(double c) { return c > 0.0 && c < HUGE_VAL; }      // (false for NaN)

__global__ void __launch_bounds__(PRICE_BLOCK)
prices_scatter_kernel(const int32_t* __restrict__ stocks, const double* __restrict__ closes, int64_t m, int64_t n_stocks,
                      int32_t* __restrict__ stamp) {
  const int64_t stride = (int64_t)gridDim.x * PRICE_BLOCK;
  for (int64_t p = (int64_t)blockIdx.x * PRICE_BLOCK + threadIdx.x; p < m; p += stride) {
    const int64_t s = stocks[p];
    if (s >= 0 && s < n_stocks && close_ok(closes[p])) atomicMax(&stamp[s], (int32_t)(p + 1));      // (m < 2^31: p + 1 fits)
  }
}

__global__ void __launch_bounds__(PRICE_BLOCK)
prices_append_kernel(const uint64_t* __restrict__ prev, uint64_t* __restrict__ next, int64_t n_stocks, int32_t n_ret,
                     const double* __restrict__ closes, int64_t n_closes, const int32_t* __restrict__ stamp,
                     double* __restrict__ last_close, int64_t* __restrict__ key_slot, int64_t day_key, double* __restrict__ quot_out) {
  const int64_t total = n_stocks * (int64_t)n_ret, stride = (int64_t)gridDim.x * PRICE_BLOCK;
  if (blockIdx.x == 0 && threadIdx.x == 0) *key_slot = day_key;
  for (int64_t i = (int64_t)blockIdx.x * PRICE_BLOCK + threadIdx.x; i < total; i += stride) {
    const int64_t s = i / n_ret;
    const int32_t j = (int32_t)(i - s * n_ret);
    if (j < n_ret - 1) {
      next[i] = prev ? prev[i + 1] : 0;                    // (i + 1 stays inside row s)
      continue;
    }
    double c = NAN;
    if (stamp) {
      const int64_t p = stamp[s];
      if (p >= 1 && p <= n_closes) c = closes[p - 1];
    } else if (s < n_closes) {
      c = closes[s];
    }
    const bool quoted = close_ok(c);
    const double last = last_close[s];
    double r = 0.0, q = NAN;
    if (quoted) {
      if (!(last != last)) {
        q = c / last;
        r = log(q);
      }
      last_close[s] = c;
    }
    reinterpret_cast<double*>(next)[i] = r;
    if (quot_out) quot_out[s] = q;
  }
}

__global__ void __launch_bounds__(PRICE_BLOCK)
prices_lookup_kernel(const double* __restrict__ ts, int64_t U, const int64_t* __restrict__ day_keys, int32_t day_cap, int32_t head,
                     int32_t n_days, double key_divisor, int32_t* __restrict__ slot_out) {
  const int64_t stride = (int64_t)gridDim.x * PRICE_BLOCK;
  for (int64_t u = (int64_t)blockIdx.x * PRICE_BLOCK + threadIdx.x; u < U; u += stride) {
    const double f = floor(ts[u] / key_divisor);
    int32_t slot = -1;
    if (f >= -9.2e18 && f <= 9.2e18) {                     // (false for NaN; the cast below is defined)
      const int64_t key = (int64_t)f;
      int32_t lo = 0, hi = n_days;                         // first live ordinal whose key is >= key
      while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        int32_t sl = head + mid;
        if (sl >= day_cap) sl -= day_cap;
        if (day_keys[sl] < key) lo = mid + 1; else hi = mid;
      }
      if (lo < n_days) {
        int32_t sl = head + lo;
        if (sl >= day_cap) sl -= day_cap;
        if (day_keys[sl] == key) slot = sl;
      }
    }
    slot_out[u] = slot;
  }
}

bool stocks_ok(int64_t n_stocks) { return n_stocks >= 0 && n_stocks < ((int64_t)1 << 31); }

}  // namespace

extern "C" int64_t pfo_returns_scatter_scratch_bytes(int64_t n_stocks) {
  if (!stocks_ok(n_stocks)) {
    pfo_set_error("%s: n_stocks must lie in [0, 2^31)", __func__);
    return -1;
  }
  return n_stocks * 4;                                     // the stamp table
}

extern "C" int pfo_returns_scatter_closes(const int32_t* stocks, const double* closes, int64_t m, int64_t n_stocks, int32_t* stamp,
                                          int64_t stamp_bytes, void* stream) {
  PFO_REQUIRE(stocks_ok(n_stocks), "n_stocks must lie in [0, 2^31)");
  PFO_REQUIRE(m >= 0 && m < ((int64_t)1 << 31), "m must lie in [0, 2^31)");
  if (n_stocks == 0) return PFO_OK;
  PFO_REQUIRE(stamp && (m == 0 || (stocks && closes)), "null pointer");
  PFO_REQUIRE(stamp_bytes >= n_stocks * 4, "short scratch");
  hipStream_t s = (hipStream_t)stream;
  PFO_REQUIRE(hipMemsetAsync(stamp, 0, (size_t)n_stocks * 4, s) == hipSuccess, "memset failed");
  if (m > 0) hipLaunchKernelGGL(prices_scatter_kernel, dim3(price_grid(m)), dim3(PRICE_BLOCK), 0, s, stocks, closes, m, n_stocks, stamp);
  PFO_LAUNCH_CHECK();
  return PFO_OK;
}

extern "C" int pfo_returns_append_day(double* returns, int32_t day_cap, int64_t stock_cap, int32_t n_ret, int32_t prev_slot,
                                      int32_t new_slot, int64_t n_stocks, const double* closes, int64_t n_closes, const int32_t* stamp,
                                      double* last_close, int64_t* day_keys, int64_t day_key, double* quot_out, void* stream) {
  PFO_REQUIRE(day_cap >= 2, "day_cap must be at least 2");
  PFO_REQUIRE(n_ret >= 2 && n_ret <= 128, "n_ret must lie in [2, 128]");
  PFO_REQUIRE(stock_cap >= 1 && stock_cap < ((int64_t)1 << 31), "stock_cap must lie in [1, 2^31)");
  PFO_REQUIRE(n_stocks >= 0 && n_stocks <= stock_cap, "n_stocks must lie in [0, stock_cap]");
  PFO_REQUIRE(new_slot >= 0 && new_slot < day_cap, "new_slot must lie in [0, day_cap)");
  PFO_REQUIRE(prev_slot >= -1 && prev_slot < day_cap, "prev_slot must lie in [-1, day_cap)");
  PFO_REQUIRE(prev_slot != new_slot, "the new slot must not be the slot it is shifted from");
  PFO_REQUIRE(n_closes >= 0 && n_closes < ((int64_t)1 << 31), "n_closes must lie in [0, 2^31)");
  PFO_REQUIRE(returns && day_keys && (n_stocks == 0 || last_close) && (n_closes == 0 || closes), "null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int64_t block = stock_cap * (int64_t)n_ret;
  const uint64_t* prev = prev_slot < 0 ? nullptr : reinterpret_cast<const uint64_t*>(returns) + prev_slot * block;
  // (n_stocks == 0: one workgroup, for the key alone)
  hipLaunchKernelGGL(prices_append_kernel, dim3(price_grid(std::max<int64_t>(n_stocks * (int64_t)n_ret, 1))), dim3(PRICE_BLOCK), 0, s, prev,
                     reinterpret_cast<uint64_t*>(returns) + new_slot * block, n_stocks, n_ret, closes, n_closes, stamp, last_close,
                     day_keys + new_slot, day_key, quot_out);
  PFO_LAUNCH_CHECK();
  return PFO_OK;
}

extern "C" int pfo_day_lookup(const double* ts, int64_t U, const int64_t* day_keys, int32_t day_cap, int32_t head, int32_t n_days,
                              double key_divisor, int32_t* slot_out, void* stream) {
  PFO_REQUIRE(U >= 0, "U must not be negative");
  PFO_REQUIRE(day_cap >= 1, "day_cap must be positive");
  PFO_REQUIRE(n_days >= 0 && n_days <= day_cap, "n_days must lie in [0, day_cap]");
  PFO_REQUIRE(head >= 0 && head < day_cap, "head must lie in [0, day_cap)");
  PFO_REQUIRE(key_divisor > 0.0 && key_divisor < HUGE_VAL, "key_divisor must be positive and finite");
  if (U == 0) return PFO_OK;
  PFO_REQUIRE(ts && day_keys && slot_out, "null pointer");
  hipLaunchKernelGGL(prices_lookup_kernel, dim3(price_grid(U)), dim3(PRICE_BLOCK), 0, (hipStream_t)stream, ts, U, day_keys, day_cap,
                     head, n_days, key_divisor, slot_out);
  PFO_LAUNCH_CHECK();
  return PFO_OK;
}
