// Holdings ledger (TGN.track_holdings / update_holdings / recommend(exclude="held", portfolios="held")): per node row the
// portfolio its newest interaction record carried - stock indices i32[W] padded with -1, their count, the record's time.
//
// Store.  The rule is a sequential loop over the events in input order, so per user the LAST event of the call owns the row.
// On the device that is the project's stamp scheme (memory.hip observe_select_kernel, the message store's winner pass) cut at
// kernel boundaries, the only hand-off between workgroups (scan64.hpp):
//   1. the stamp table i32[n_nodes] is cleared (one memset node);
//   2. every event with a valid user stamps it: atomicMax(stamp[u], e + 1) - integer maxima commute, so the table is the same
//      whatever the launch geometry and the arrival order;
//   3. one lane per ELEMENT of the [N, W] block: the lanes of event e whose stamp[u] == e + 1 copy the row, consecutive lanes
//      on consecutive addresses of both the input row and the ledger row; the lane of column 0 also writes length and time.
//      Losing events write nothing, rows of users the call does not name are not touched.
// Stamps of one call never decide another: the table is cleared per call (n_nodes * 4 bytes - 200 KB at 50 k nodes).
//
// Gather.  Query rows by user, and - for `exclude` - their stocks as POSITIONS in the query's candidate list.  The node id ->
// position table over the node ids is never cleared: the scatter writes pos[items[i]] = i, and a reader trusts pos[v] = p only
// if 0 <= p < I and items[p] == v.  An entry of an earlier candidate list (or of uninitialised memory) either fails that test
// or names a position that holds v in THIS list - where, the candidates being distinct, this call's scatter wrote the same p.
// Two launches, no fill over n_nodes per query.
//
// Every index that comes from device memory is range-checked before it addresses anything: users and event sources against
// [0, n_nodes), lengths clamped to the row, stock indices against the node table BEFORE upper_u + 1 is added.
#include "common.hpp"
#include <algorithm>

namespace {

constexpr int HOLD_BLOCK = 256;
constexpr int64_t HOLD_MAX_GRID = 1 << 20;       // beyond that the lanes stride

unsigned hold_grid(int64_t total) { return (unsigned)std::min<int64_t>(pfo_ceil_div(total, HOLD_BLOCK), HOLD_MAX_GRID); }

__global__ void __launch_bounds__(HOLD_BLOCK)
holdings_stamp_kernel(const int32_t* __restrict__ src, int64_t N, int64_t n_nodes, int32_t* __restrict__ stamp) {
  const int64_t stride = (int64_t)gridDim.x * HOLD_BLOCK;
  for (int64_t e = (int64_t)blockIdx.x * HOLD_BLOCK + threadIdx.x; e < N; e += stride) {
    const int64_t u = src[e];
    if (u >= 1 && u < n_nodes) atomicMax(&stamp[u], (int32_t)(e + 1));       // (N < 2^31: e + 1 fits)
  }
}

__global__ void __launch_bounds__(HOLD_BLOCK)
holdings_copy_kernel(const int32_t* __restrict__ src, const int32_t* __restrict__ port_idx, const int32_t* __restrict__ port_len,
                     int32_t port_stride, const double* __restrict__ ts, int64_t N, int32_t* __restrict__ hold_idx,
                     int32_t* __restrict__ hold_len, double* __restrict__ hold_time, int64_t n_nodes, int32_t W,
                     const int32_t* __restrict__ stamp) {
  const int64_t total = N * (int64_t)W, stride = (int64_t)gridDim.x * HOLD_BLOCK;
  const int32_t row_max = std::min(W, port_stride);
  for (int64_t i = (int64_t)blockIdx.x * HOLD_BLOCK + threadIdx.x; i < total; i += stride) {
    const int64_t e = i / W;
    const int32_t j = (int32_t)(i - e * W);
    const int64_t u = src[e];
    if (u < 1 || u >= n_nodes) continue;                   // skipped: nothing written
    if (stamp[u] != (int32_t)(e + 1)) continue;            // a later event of this call names u
    const int32_t L = std::min(std::max(port_len[e], 0), row_max);
    hold_idx[u * W + j] = j < L ? port_idx[e * (int64_t)port_stride + j] : -1;
    if (j == 0) {
      hold_len[u] = L;
      hold_time[u] = ts[e];
    }
  }
}

__global__ void __launch_bounds__(HOLD_BLOCK)
holdings_pos_kernel(const int32_t* __restrict__ items, int32_t I, int64_t n_nodes, int32_t* __restrict__ pos) {
  const int32_t i = blockIdx.x * HOLD_BLOCK + threadIdx.x;
  if (i >= I) return;
  const int64_t v = items[i];
  if (v >= 0 && v < n_nodes) pos[v] = i;
}

__global__ void __launch_bounds__(HOLD_BLOCK)
holdings_gather_kernel(const int32_t* __restrict__ users, int64_t U, const int32_t* __restrict__ hold_idx,
                       const int32_t* __restrict__ hold_len, int64_t n_nodes, int32_t W, const int32_t* __restrict__ items, int32_t I,
                       int32_t upper_u, const int32_t* __restrict__ pos, int32_t* __restrict__ port_idx_out,
                       int32_t* __restrict__ port_len_out, int32_t* __restrict__ excl_pos_out) {
  const int64_t total = U * (int64_t)W, stride = (int64_t)gridDim.x * HOLD_BLOCK;
  const int64_t shift = (int64_t)upper_u + 1;              // item node of stock s: s + upper_u + 1
  for (int64_t i = (int64_t)blockIdx.x * HOLD_BLOCK + threadIdx.x; i < total; i += stride) {
    const int64_t q = i / W;
    const int32_t j = (int32_t)(i - q * W);
    const int64_t u = users[q];
    const bool ok = u >= 0 && u < n_nodes;
    const int32_t s = ok ? hold_idx[u * W + j] : -1;
    const int32_t len = ok ? hold_len[u] : 0;
    port_idx_out[i] = s;
    if (j == 0) port_len_out[q] = len;
    if (excl_pos_out) {
      int32_t p = -1;
      // the stock index is checked against the node table first: s + shift is then a node id, nothing overflows
      if (j < len && s >= 0 && (int64_t)s < n_nodes - shift && (int64_t)s + shift >= 0) {
        const int64_t node = (int64_t)s + shift;
        const int32_t c = pos[node];
        if (c >= 0 && c < I && items[c] == node) p = c;    // (an entry of an earlier list fails this, or is right)
      }
      excl_pos_out[i] = p;
    }
  }
}

bool hold_sizes_ok(int64_t n_nodes, int32_t W) { return n_nodes >= 1 && n_nodes < ((int64_t)1 << 31) && W >= 1 && W <= 256; }

}  // namespace

extern "C" int64_t pfo_holdings_store_scratch_bytes(int64_t n_nodes, int64_t N) {
  if (n_nodes < 1 || n_nodes >= ((int64_t)1 << 31) || N < 0 || N >= ((int64_t)1 << 31)) {
    pfo_set_error("%s: n_nodes must lie in [1, 2^31) and N in [0, 2^31)", __func__);
    return -1;
  }
  return n_nodes * 4;                                      // the stamp table
}

extern "C" int pfo_holdings_store(const int32_t* src, const int32_t* port_idx, const int32_t* port_len, int32_t port_stride,
                                  const double* ts, int64_t N, int32_t* hold_idx, int32_t* hold_len, double* hold_time,
                                  int64_t n_nodes, int32_t W, void* scratch, int64_t scratch_bytes, void* stream) {
  PFO_REQUIRE(W >= 1 && W <= 256, "W must lie in [1, 256]");
  PFO_REQUIRE(N >= 0 && N < ((int64_t)1 << 31), "N must lie in [0, 2^31)");
  PFO_REQUIRE(n_nodes >= 1 && n_nodes < ((int64_t)1 << 31), "n_nodes must lie in [1, 2^31)");
  PFO_REQUIRE(port_stride >= 0, "port_stride must not be negative");
  if (N == 0) return PFO_OK;
  PFO_REQUIRE(src && port_len && ts && hold_idx && hold_len && hold_time && scratch && (port_idx || port_stride == 0), "null pointer");
  PFO_REQUIRE(scratch_bytes >= n_nodes * 4, "short scratch");
  hipStream_t s = (hipStream_t)stream;
  int32_t* stamp = reinterpret_cast<int32_t*>(scratch);
  PFO_REQUIRE(hipMemsetAsync(stamp, 0, (size_t)n_nodes * 4, s) == hipSuccess, "memset failed");
  hipLaunchKernelGGL(holdings_stamp_kernel, dim3(hold_grid(N)), dim3(HOLD_BLOCK), 0, s, src, N, n_nodes, stamp);
  hipLaunchKernelGGL(holdings_copy_kernel, dim3(hold_grid(N * (int64_t)W)), dim3(HOLD_BLOCK), 0, s, src, port_idx, port_len, port_stride,
                     ts, N, hold_idx, hold_len, hold_time, n_nodes, W, (const int32_t*)stamp);
  PFO_LAUNCH_CHECK();
  return PFO_OK;
}

extern "C" int pfo_holdings_gather(const int32_t* users, int64_t U, const int32_t* hold_idx, const int32_t* hold_len, int64_t n_nodes,
                                   int32_t W, const int32_t* items, int32_t I, int32_t upper_u, int32_t* pos_scratch,
                                   int32_t* port_idx_out, int32_t* port_len_out, int32_t* excl_pos_out, void* stream) {
  PFO_REQUIRE(W >= 1 && W <= 256, "W must lie in [1, 256]");
  PFO_REQUIRE(I >= 1 && I <= PFO_RECOMMEND_MAX_ITEMS, "I must lie in [1, PFO_RECOMMEND_MAX_ITEMS]");
  PFO_REQUIRE(n_nodes >= 1 && n_nodes < ((int64_t)1 << 31), "n_nodes must lie in [1, 2^31)");
  PFO_REQUIRE(U >= 0 && U <= INT64_MAX / 256, "U must not be negative");
  if (U == 0) return PFO_OK;
  PFO_REQUIRE(users && hold_idx && hold_len && port_idx_out && port_len_out, "null pointer");
  PFO_REQUIRE(!excl_pos_out || (items && pos_scratch), "null pointer: positions need items and pos_scratch");
  hipStream_t s = (hipStream_t)stream;
  if (excl_pos_out)
    hipLaunchKernelGGL(holdings_pos_kernel, dim3((unsigned)pfo_ceil_div(I, HOLD_BLOCK)), dim3(HOLD_BLOCK), 0, s, items, I, n_nodes,
                       pos_scratch);
  hipLaunchKernelGGL(holdings_gather_kernel, dim3(hold_grid(U * (int64_t)W)), dim3(HOLD_BLOCK), 0, s, users, U, hold_idx, hold_len, n_nodes,
                     W, items, I, upper_u, (const int32_t*)pos_scratch, port_idx_out, port_len_out, excl_pos_out);
  PFO_LAUNCH_CHECK();
  return PFO_OK;
}
