// History gather (TGN.history / recommend(exclude="seen", only="seen", portfolios="seen")): per query (user, time) the DISTINCT
// neighbours the user's row of the temporal adjacency names strictly before that time, newest first - read from the time-sorted
// CSR the finder keeps on the device anyway (indptr i64, adj_nbr i32, adj_ts f64).  Semantics: include/pfotgn.h.
//
// One user per 64-thread workgroup.  A workgroup is ONE wavefront, so every loop below - the search steps, the chunk walk, the
// scan of the kept list - has a trip count all its lanes agree on (it is derived from ballots and from values every lane
// loaded from the same address), and the __syncthreads() inside them are legal.  With four users per 256 threads the
// wavefronts of a workgroup would walk rows of different lengths and disagree on how many barriers they meet.
//
//   bounds : a 64-ary lower bound on adj_ts over the row: the lanes probe 64 split points, a ballot and a popcount pick the
//            sub-range - the range shrinks by 64 per step, 3 steps for a row of 20 000 entries.  fp64 compares on the stored
//            fp64 timestamps: expire's rule, none of the sampler's fp32 casts.
//   walk   : chunks of 64 entries newest first; lane j reads entry hi - 1 - (64 c + j) (contiguous, descending).  A lane is a
//            repeat inside the chunk if a lower lane holds its id, a repeat against the kept list by broadcast reads of the kept
//            ids in LDS (at most 256).  New ids take slots kept + rank among the chunk's new ids (ballot, prefix popcount).
//            Counts are integer adds into the slot's LDS word: order-free, the same on every run.
//   out    : one slot per lane and pass, plain vector stores, padding included.  No float atomics, no global atomics.
//
// Every index that comes from device memory is range-checked before it addresses anything: users against [0, n_nodes), a
// neighbour id against [0, n_nodes) before it indexes pos_scratch, a position against [0, I) before it indexes items.
#include "common.hpp"
#include <algorithm>

namespace {

constexpr int HIST_BLOCK = 64;                   // one wavefront: see above
constexpr int64_t HIST_MAX_GRID = 1 << 20;       // beyond that the workgroups stride over the users
constexpr int HIST_POS_BLOCK = 256;

__global__ void __launch_bounds__(HIST_POS_BLOCK)
history_pos_kernel(const int32_t* __restrict__ items, int32_t I, int64_t n_nodes, int32_t* __restrict__ pos) {
  const int32_t i = blockIdx.x * HIST_POS_BLOCK + threadIdx.x;
  if (i >= I) return;
  const int64_t v = items[i];
  if (v >= 0 && v < n_nodes) pos[v] = i;
}

// the number of entries of t[0, n) (ascending) that are < key; every lane of the wavefront returns the same value
__device__ __forceinline__ int64_t hist_lower_bound(const double* __restrict__ t, int64_t n, double key, int lane) {
  int64_t lo = 0, hi = n;                        // the answer lies in [lo, hi]
  while (hi - lo > HIST_BLOCK) {
    const int64_t step = (hi - lo + HIST_BLOCK - 1) / HIST_BLOCK;
    const int64_t p = lo + (int64_t)(lane + 1) * step - 1;
    const int c = (int)__popcll(__ballot(p < hi && t[p] < key));          // (sorted: the lanes that say yes are a prefix)
    const int64_t nlo = lo + (int64_t)c * step;
    hi = std::min(hi, nlo + step - 1);           // (probe c, if it lies in the row, is >= key)
    lo = nlo;
  }
  return lo + (int)__popcll(__ballot(lo + lane < hi && t[lo + lane] < key));
}

__global__ void __launch_bounds__(HIST_BLOCK)
history_gather_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ adj_nbr, const double* __restrict__ adj_ts,
                      int64_t n_nodes, const int32_t* __restrict__ users, const double* __restrict__ ts,
                      const double* __restrict__ since, int64_t U, int32_t W, int64_t max_scan, const int32_t* __restrict__ items,
                      int32_t I, const int32_t* __restrict__ pos, int32_t upper_u, int32_t* __restrict__ node_out,
                      int32_t* __restrict__ len_out, double* __restrict__ time_out, int32_t* __restrict__ count_out,
                      int32_t* __restrict__ pos_out, int32_t* __restrict__ stock_out) {
  __shared__ int32_t s_id[PFO_HISTORY_MAX_WIDTH];
  __shared__ int32_t s_cnt[PFO_HISTORY_MAX_WIDTH];
  __shared__ double s_time[PFO_HISTORY_MAX_WIDTH];
  const int lane = threadIdx.x;
  const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
  for (int64_t q = blockIdx.x; q < U; q += gridDim.x) {
    const int64_t u = users[q];
    const double t = ts[q];
    int kept = 0;
    if (u >= 0 && u < n_nodes && isfinite(t)) {
      const int64_t base = indptr[u];
      const int64_t n = std::max<int64_t>(indptr[u + 1] - base, 0);
      const double* __restrict__ row_ts = adj_ts + base;
      const int32_t* __restrict__ row_nbr = adj_nbr + base;
      const int64_t hi = hist_lower_bound(row_ts, n, t, lane);
      int64_t lo = 0;
      if (since) {
        const double s = since[q];
        if (!isnan(s)) lo = hist_lower_bound(row_ts, n, s, lane);
      }
      if (max_scan > 0) lo = std::max(lo, hi - max_scan);
      for (int64_t top = hi; top > lo; top -= HIST_BLOCK) {          // entries [lo, top) are still to be walked
        if (kept >= W && !count_out) break;                          // the list is full and nobody counts
        const int64_t e = top - 1 - lane;
        const bool active = e >= lo;
        const int32_t id = active ? row_nbr[e] : 0;
        const double et = active ? row_ts[e] : 0.0;
        const unsigned long long act = __ballot(active);
        bool dup = false;                                            // a lower lane of the chunk holds the same id
        for (int j = 0; j < HIST_BLOCK - 1; ++j) {
          const int32_t other = __shfl(id, j);
          dup |= j < lane && ((act >> j) & 1) && other == id;
        }
        int slot = -1;                                               // against the kept list: broadcast reads
        for (int i = 0; i < kept; ++i)
          if (s_id[i] == id) slot = i;
        const bool fresh = active && !dup && slot < 0;
        const unsigned long long fresh_mask = __ballot(fresh);
        const int mine = kept + (int)__popcll(fresh_mask & below);
        if (fresh && mine < W) {                                     // (a first meeting behind W slots is dropped)
          s_id[mine] = id;
          s_time[mine] = et;
          s_cnt[mine] = 0;
        }
        const int kept_new = std::min(kept + (int)__popcll(fresh_mask), (int)W);
        __syncthreads();
        if (active && slot < 0)                                      // this chunk's own first meetings, and their repeats
          for (int i = kept; i < kept_new; ++i)
            if (s_id[i] == id) slot = i;
        if (active && slot >= 0) atomicAdd(&s_cnt[slot], 1);         // (LDS integer add: order-free)
        kept = kept_new;
        __syncthreads();
      }
    }
    __syncthreads();
    for (int p = lane; p < W; p += HIST_BLOCK) {
      const bool valid = p < kept;
      const int64_t o = q * (int64_t)W + p;
      const int32_t v = valid ? s_id[p] : -1;
      node_out[o] = v;
      if (time_out) time_out[o] = valid ? s_time[p] : __longlong_as_double(0x7ff8000000000000ll);
      if (count_out) count_out[o] = valid ? s_cnt[p] : 0;
      if (pos_out) {
        int32_t c = -1;
        if (valid && v >= 0 && (int64_t)v < n_nodes) {
          const int32_t cand = pos[v];
          if (cand >= 0 && cand < I && items[cand] == v) c = cand;   // (an entry of an earlier list fails this, or is right)
        }
        pos_out[o] = c;
      }
      if (stock_out) {
        const int64_t s = (int64_t)v - (int64_t)upper_u - 1;         // (64-bit: nothing wraps before the range check)
        stock_out[o] = valid && s >= 0 && s < ((int64_t)1 << 31) ? (int32_t)s : -1;
      }
    }
    if (lane == 0) len_out[q] = kept;
    __syncthreads();                                                 // the next user's walk rewrites the LDS rows
  }
}

}  // namespace

extern "C" int pfo_history_gather(const int64_t* indptr, const int32_t* adj_nbr, const double* adj_ts, int64_t n_nodes,
                                  const int32_t* users, const double* ts, const double* since, int64_t U, int32_t W,
                                  int64_t max_scan, const int32_t* items, int32_t I, int32_t* pos_scratch, int32_t upper_u,
                                  int32_t* node_out, int32_t* len_out, double* time_out, int32_t* count_out, int32_t* pos_out,
                                  int32_t* stock_out, void* stream) {
  PFO_REQUIRE(W >= 1 && W <= PFO_HISTORY_MAX_WIDTH, "W must lie in [1, PFO_HISTORY_MAX_WIDTH]");
  PFO_REQUIRE(U >= 0 && U <= INT64_MAX / PFO_HISTORY_MAX_WIDTH, "U must lie in [0, INT64_MAX / PFO_HISTORY_MAX_WIDTH]");
  PFO_REQUIRE(n_nodes >= 1 && n_nodes < ((int64_t)1 << 31), "n_nodes must lie in [1, 2^31)");
  PFO_REQUIRE(max_scan >= 0, "max_scan must not be negative");
  PFO_REQUIRE(!pos_out || (I >= 1 && I <= PFO_RECOMMEND_MAX_ITEMS), "with pos_out, I must lie in [1, PFO_RECOMMEND_MAX_ITEMS]");
  if (U == 0) return PFO_OK;
  PFO_REQUIRE(indptr && adj_nbr && adj_ts && users && ts && node_out && len_out, "null pointer");
  PFO_REQUIRE(!pos_out || (items && pos_scratch), "null pointer: positions need items and pos_scratch");
  hipStream_t s = (hipStream_t)stream;
  if (pos_out)
    hipLaunchKernelGGL(history_pos_kernel, dim3((unsigned)pfo_ceil_div(I, HIST_POS_BLOCK)), dim3(HIST_POS_BLOCK), 0, s, items, I,
                       n_nodes, pos_scratch);
  hipLaunchKernelGGL(history_gather_kernel, dim3((unsigned)std::min<int64_t>(U, HIST_MAX_GRID)), dim3(HIST_BLOCK), 0, s, indptr,
                     adj_nbr, adj_ts, n_nodes, users, ts, since, U, W, max_scan, items, I, (const int32_t*)pos_scratch, upper_u,
                     node_out, len_out, time_out, count_out, pos_out, stock_out);
  PFO_LAUNCH_CHECK();
  return PFO_OK;
}
