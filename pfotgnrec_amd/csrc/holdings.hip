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
//
// Apply (holdings from trades).  The rule is again a sequential loop over the events in input order, but here every
// event of a user matters, not the last one alone.  1. The events are grouped by user, stable in input order: key[e] = the user
// of a valid event, 0 of an invalid one, and the event indices are placed by a stable LSD radix over the key, 8 bits a pass,
// ceil(log256(n_nodes)) passes, keys never moving (the scheme of csr.hip, its pass kernels' siblings below; a call of one tile
// - a serving tick - groups in LDS in one launch of one wavefront).  2. One wavefront per sorted position; the one at the head
// of a user's chain loads the row into registers (slot s in lane s & 63), walks the chain - 64 events read at a time, then one
// by one by broadcast: a ballot per 64 slots finds the first occurrence, the owner lane appends or adds, a close shifts by
// shuffle with one carry between the 64-slot pieces - and writes row, length and time once.  No per-user count and no scan
// over the node rows: the chain ends where the key changes, so the work follows N and never n_nodes.  The result is the
// loop's whatever the launch geometry: a chain has one owner, and only the two integer counters meet in atomics.
#include "memory.hpp"
#include <algorithm>

#define TR_TILE 1024        // events per wavefront tile of a radix pass (16 steps of 64)
#define TR_STEPS (TR_TILE / 64)

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

// ------------------------------------------------------------------------------------------------ apply: holdings from trades
// key of event e: its user when the event is valid, 0 otherwise (node 0 is never a user: the invalid events sort in front of
// every chain and no wavefront walks them)
__device__ __forceinline__ bool trade_ok(int64_t u, int32_t stock, int32_t side, bool has_q, double q, int64_t n_nodes) {
  return u >= 1 && u < n_nodes && stock >= 0 && (side == 1 || side == -1) && (!has_q || (q > 0.0 && q <= 1.79769313486231570815e308));
}

__global__ void __launch_bounds__(HOLD_BLOCK)
trades_key_kernel(const int32_t* __restrict__ src, const int32_t* __restrict__ stock, const int32_t* __restrict__ side,
                  const double* __restrict__ qty, int64_t N, int64_t n_nodes, int32_t* __restrict__ key, int32_t* __restrict__ perm) {
  const int64_t stride = (int64_t)gridDim.x * HOLD_BLOCK;
  for (int64_t e = (int64_t)blockIdx.x * HOLD_BLOCK + threadIdx.x; e < N; e += stride) {
    const int32_t u = src[e];
    key[e] = trade_ok(u, stock[e], side[e], qty != nullptr, qty ? qty[e] : 1.0, n_nodes) ? u : 0;
    perm[e] = (int32_t)e;
  }
}

__device__ __forceinline__ int trade_digit(const int32_t* key, int32_t e, int64_t N, int shift) {
  return (e >= 0 && e < N) ? (int)(((uint32_t)key[e] >> shift) & 255u) : 0;
}

// one pass of the stable LSD radix over the user id (the scheme of csr.hip: 1024-entry tiles, one wavefront each, same-digit lanes
// ranked by ballots in input order; the keys never move): per-tile digit histogram, digit-major
__global__ void __launch_bounds__(64)
trades_hist_kernel(const int32_t* __restrict__ key, const int32_t* __restrict__ perm, int64_t N, int shift, int32_t* __restrict__ hist,
                   int n_tiles) {
  __shared__ int s_cnt[256];
  const int lane = threadIdx.x;
  for (int d = lane; d < 256; d += 64) s_cnt[d] = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * TR_TILE;
  for (int st = 0; st < TR_STEPS; ++st) {
    const int64_t i = base + st * 64 + lane;
    if (i < N) atomicAdd(&s_cnt[trade_digit(key, perm[i], N, shift)], 1);
  }
  __syncthreads();
  for (int d = lane; d < 256; d += 64) hist[(int64_t)d * n_tiles + blockIdx.x] = s_cnt[d];
}

// the tile's 16 steps of 64 in order; `s_off[d]` is where the tile's next entry of digit d goes.  Barriers stand in the
// uniform step loop, outside every lane's branch.
template <typename Out>
__device__ __forceinline__ void trades_scatter_tile(const int32_t* key, const int32_t* perm_in, int64_t t0, int64_t N, int shift, int* s_off,
                                                    Out out, int64_t out_n, int lane) {
  for (int st = 0; st < TR_STEPS; ++st) {
    const int64_t i = t0 + st * 64 + lane;
    const bool live = i < N;
    const int32_t idx = live ? perm_in[i] : 0;
    const int d = live ? trade_digit(key, idx, N, shift) : 0;
    unsigned long long same = __ballot(live);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const unsigned long long bal = __ballot(live && ((d >> b) & 1));
      same &= ((d >> b) & 1) ? bal : ~bal;
    }
    const int rank = __popcll(same & ((1ull << lane) - 1ull));
    int off = 0;
    if (live) off = s_off[d];
    const int64_t o = (int64_t)off + rank;
    if (live && o >= 0 && o < out_n) out[o] = idx;
    __syncthreads();
    if (live && rank == 0) s_off[d] = off + __popcll(same);
    __syncthreads();
  }
}

__global__ void __launch_bounds__(64)
trades_scatter_kernel(const int32_t* __restrict__ key, const int32_t* __restrict__ perm, int64_t N, int shift,
                      const int32_t* __restrict__ base, int n_tiles, int32_t* __restrict__ out) {
  __shared__ int s_off[256];
  const int lane = threadIdx.x;
  for (int d = lane; d < 256; d += 64) s_off[d] = base[(int64_t)d * n_tiles + blockIdx.x];
  __syncthreads();
  trades_scatter_tile(key, perm, (int64_t)blockIdx.x * TR_TILE, N, shift, s_off, out, N, lane);
}

// a call of one tile (N <= 1024: the serving tick): keys, every radix pass and the permutation in ONE launch of one wavefront,
// the two permutation images and the digit offsets in LDS (13 KB)
__global__ void __launch_bounds__(64)
trades_group_small_kernel(const int32_t* __restrict__ src, const int32_t* __restrict__ stock, const int32_t* __restrict__ side,
                          const double* __restrict__ qty, int32_t N, int64_t n_nodes, int passes, int32_t* __restrict__ key,
                          int32_t* __restrict__ perm) {
  __shared__ int32_t s_key[TR_TILE];
  __shared__ int32_t s_perm[2][TR_TILE];
  __shared__ int s_off[256];
  const int lane = threadIdx.x;
  for (int i = lane; i < N; i += 64) {
    const int32_t u = src[i];
    const int32_t k = trade_ok(u, stock[i], side[i], qty != nullptr, qty ? qty[i] : 1.0, n_nodes) ? u : 0;
    s_key[i] = k;
    key[i] = k;
    s_perm[0][i] = i;
  }
  __syncthreads();
  int cur = 0;
  for (int p = 0; p < passes; ++p) {
    const int shift = 8 * p;
    for (int d = lane; d < 256; d += 64) s_off[d] = 0;
    __syncthreads();
    for (int i = lane; i < N; i += 64) atomicAdd(&s_off[trade_digit(s_key, s_perm[cur][i], N, shift)], 1);
    __syncthreads();
    // exclusive scan of the 256 counts: four consecutive digits a lane, a shuffle scan over the lane sums
    const int a0 = s_off[4 * lane], a1 = s_off[4 * lane + 1], a2 = s_off[4 * lane + 2], a3 = s_off[4 * lane + 3];
    const int sum = a0 + a1 + a2 + a3;
    int incl = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(incl, o, 64);
      if (lane >= o) incl += v;
    }
    const int excl = incl - sum;
    __syncthreads();
    s_off[4 * lane] = excl;
    s_off[4 * lane + 1] = excl + a0;
    s_off[4 * lane + 2] = excl + a0 + a1;
    s_off[4 * lane + 3] = excl + a0 + a1 + a2;
    __syncthreads();
    trades_scatter_tile(s_key, s_perm[cur], 0, N, shift, s_off, s_perm[cur ^ 1], (int64_t)N, lane);
    cur ^= 1;
  }
  for (int i = lane; i < N; i += 64) perm[i] = s_perm[cur][i];
}

// One wavefront per sorted position; the one that stands at the HEAD of a user's chain (the entry in front of it has another
// key) walks the chain, every other wavefront leaves after two loads.  NP = pieces of 64 slots a row takes (W <= 64 NP): slot
// s of the row lives in lane s & 63, piece s >> 6, in registers for the whole walk.  No workgroup barrier, no LDS; every
// store is a plain vector store at the end.
template <int NP, bool QTY>
__global__ void __launch_bounds__(HOLD_BLOCK)
trades_apply_kernel(const int32_t* __restrict__ key, const int32_t* __restrict__ perm, const int32_t* __restrict__ stock,
                    const int32_t* __restrict__ side, const double* __restrict__ qty, const double* __restrict__ ts, int64_t N,
                    int32_t* __restrict__ hold_idx, int32_t* __restrict__ hold_len, double* __restrict__ hold_time,
                    double* __restrict__ hold_qty, int64_t n_nodes, int32_t W, unsigned long long* __restrict__ counters) {
  const int lane = threadIdx.x & 63;
  const int64_t n_waves = (int64_t)gridDim.x * (HOLD_BLOCK / 64);
  for (int64_t i0 = (int64_t)blockIdx.x * (HOLD_BLOCK / 64) + (threadIdx.x >> 6); i0 < N; i0 += n_waves) {   // (wave-uniform)
    const int32_t e0 = perm[i0];
    if (e0 < 0 || e0 >= N) continue;
    const int64_t u = key[e0];
    if (u < 1 || u >= n_nodes) continue;                   // an invalid event (key 0), or a key that is no row
    if (i0 > 0) {
      const int32_t ep = perm[i0 - 1];
      if (ep >= 0 && ep < N && key[ep] == (int32_t)u) continue;     // not the head of its chain
    }
    // load: the row, once
    int32_t ri[NP];
    double rq[NP];
    const int32_t len0 = hold_len[u];
    int L = std::min(std::max(len0, 0), W);
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int s = p * 64 + lane;
      ri[p] = s < W ? hold_idx[u * W + s] : -1;
      rq[p] = (QTY && s < W) ? hold_qty[u * W + s] : 0.0;
    }
    unsigned long long n_over = 0, n_unm = 0;
    bool any = false, len_dirty = false;
    double t_last = 0.0;
    // walk: 64 events at a time through the grouped order, then one by one by broadcast
    for (int64_t base = i0; base < N; base += 64) {
      const int64_t i = base + lane;
      const int32_t e = i < N ? perm[i] : -1;
      const bool mine = e >= 0 && e < N && key[e] == (int32_t)u;
      const unsigned long long not_mine = ~__ballot(mine);
      const int cnt = not_mine ? __ffsll((long long)not_mine) - 1 : 64;       // the chain's entries among these 64: a prefix
      const bool on = lane < cnt;
      const int32_t my_stock = on ? stock[e] : -1, my_side = on ? side[e] : 0;
      const double my_q = (on && QTY && qty) ? qty[e] : 1.0, my_t = on ? ts[e] : 0.0;
      for (int t = 0; t < cnt; ++t) {
        const int32_t s = __shfl(my_stock, t, 64), sd = __shfl(my_side, t, 64);
        const double q = QTY ? __shfl(my_q, t, 64) : 1.0;
        // (the key says the event is valid; the test is made again on what this kernel itself loaded)
        if (s < 0 || (sd != 1 && sd != -1) || !(q > 0.0 && q <= 1.79769313486231570815e308)) continue;
        any = true;
        t_last = __shfl(my_t, t, 64);
        int j = -1;                                         // the first slot of r[:L] that holds s
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          const unsigned long long hit = __ballot(p * 64 + lane < L && ri[p] == s);
          if (j < 0 && hit) j = p * 64 + __ffsll((long long)hit) - 1;
        }
        if (sd == 1) {
          if (j >= 0) {
            if (QTY) {
#pragma unroll
              for (int p = 0; p < NP; ++p)
                if (p * 64 + lane == j) rq[p] += q;
            }
          } else if (L < W) {
#pragma unroll
            for (int p = 0; p < NP; ++p)
              if (p * 64 + lane == L) { ri[p] = s; rq[p] = q; }
            ++L;
            len_dirty = true;
          } else {
            ++n_over;
          }
          continue;
        }
        if (j < 0) { ++n_unm; continue; }
        if (QTY) {
          double cur = 0.0;
#pragma unroll
          for (int p = 0; p < NP; ++p) {
            const double v = __shfl(rq[p], j & 63, 64);
            if (p == (j >> 6)) cur = v;
          }
          const double rem = cur - q;
          if (rem > 0.0) {
#pragma unroll
            for (int p = 0; p < NP; ++p)
              if (p * 64 + lane == j) rq[p] = rem;
            continue;
          }
        }
        // close: slots j+1 .. L-1 move one to the front (lane l takes lane l + 1's, lane 63 the next piece's lane 0), slot L-1
        // becomes (-1, 0.0)
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          const int32_t carry_i = p + 1 < NP ? __shfl(ri[p + 1 < NP ? p + 1 : p], 0, 64) : -1;
          int32_t nxt_i = __shfl_down(ri[p], 1, 64);
          if (lane == 63) nxt_i = carry_i;
          double nxt_q = 0.0;
          if (QTY) {
            const double carry_q = p + 1 < NP ? __shfl(rq[p + 1 < NP ? p + 1 : p], 0, 64) : 0.0;
            nxt_q = __shfl_down(rq[p], 1, 64);
            if (lane == 63) nxt_q = carry_q;
          }
          const int sl = p * 64 + lane;
          if (sl >= j && sl < L - 1) { ri[p] = nxt_i; rq[p] = nxt_q; }
          else if (sl == L - 1) { ri[p] = -1; rq[p] = 0.0; }
        }
        --L;
        len_dirty = true;
      }
      if (cnt < 64) break;
    }
    if (!any) continue;
    // write back, once
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int s = p * 64 + lane;
      if (s < W) {
        hold_idx[u * W + s] = ri[p];
        if (QTY) hold_qty[u * W + s] = rq[p];
      }
    }
    if (lane == 0) {
      if (len_dirty) hold_len[u] = L;
      hold_time[u] = t_last;
      if (counters && n_over) atomicAdd(&counters[0], n_over);
      if (counters && n_unm) atomicAdd(&counters[1], n_unm);
    }
  }
}

int trades_passes(int64_t n_nodes) {
  int bits = 1;
  while (((int64_t)1 << bits) < n_nodes) ++bits;
  return (bits + 7) / 8;
}
struct TradesScratch { int64_t key, perm0, perm1, hist, base, scan, total; };
TradesScratch trades_scratch_of(int64_t N) {
  const int64_t tiles = std::max<int64_t>(1, pfo_ceil_div(N, TR_TILE)), hist_n = tiles > 1 ? 256 * tiles : 0;
  TradesScratch s;
  int64_t b = 0;
  auto take = [&](int64_t bytes) { const int64_t at = b; b += pfo_align_up(bytes, 256); return at; };
  s.key = take(N * 4);
  s.perm0 = take(N * 4);
  s.perm1 = take(tiles > 1 ? N * 4 : 0);                   // (one tile sorts in LDS)
  s.hist = take(hist_n * 4);
  s.base = take(hist_n * 4);
  s.scan = take(hist_n ? (pfo_ceil_div(hist_n, 1024) + 16) * 4 : 0);
  s.total = b;
  return s;
}

}  // namespace

extern "C" int64_t pfo_holdings_apply_scratch_bytes(int64_t n_nodes, int64_t N) {
  if (n_nodes < 1 || n_nodes >= ((int64_t)1 << 31) || N < 0 || N >= ((int64_t)1 << 31)) {
    pfo_set_error("%s: n_nodes must lie in [1, 2^31) and N in [0, 2^31)", __func__);
    return -1;
  }
  return trades_scratch_of(N).total;
}

extern "C" int pfo_holdings_apply(const int32_t* src, const int32_t* stock, const int32_t* side, const double* qty, const double* ts,
                                  int64_t N, int32_t* hold_idx, int32_t* hold_len, double* hold_time, double* hold_qty, int64_t n_nodes,
                                  int32_t W, int64_t* counters, void* scratch, int64_t scratch_bytes, void* stream) {
  PFO_REQUIRE(W >= 1 && W <= 256, "W must lie in [1, 256]");
  PFO_REQUIRE(N >= 0 && N < ((int64_t)1 << 31), "N must lie in [0, 2^31)");
  PFO_REQUIRE(n_nodes >= 1 && n_nodes < ((int64_t)1 << 31), "n_nodes must lie in [1, 2^31)");
  if (N == 0) return PFO_OK;
  PFO_REQUIRE(src && stock && side && ts && hold_idx && hold_len && hold_time && scratch, "null pointer");
  const TradesScratch lay = trades_scratch_of(N);
  PFO_REQUIRE(scratch_bytes >= lay.total, "short scratch");
  hipStream_t s = (hipStream_t)stream;
  char* p = reinterpret_cast<char*>(scratch);
  int32_t* key = (int32_t*)(p + lay.key);
  int32_t* perm[2] = {(int32_t*)(p + lay.perm0), (int32_t*)(p + lay.perm1)};
  const double* q_in = hold_qty ? qty : nullptr;           // without quantities in the ledger the events' are ignored
  const int passes = trades_passes(n_nodes);
  const int64_t tiles = pfo_ceil_div(N, TR_TILE);
  int cur = 0;
  if (tiles == 1) {
    hipLaunchKernelGGL(trades_group_small_kernel, dim3(1), dim3(64), 0, s, src, stock, side, q_in, (int32_t)N, n_nodes, passes, key, perm[0]);
  } else {
    int32_t* hist = (int32_t*)(p + lay.hist);
    int32_t* base = (int32_t*)(p + lay.base);
    int32_t* scan = (int32_t*)(p + lay.scan);
    hipLaunchKernelGGL(trades_key_kernel, dim3(hold_grid(N)), dim3(HOLD_BLOCK), 0, s, src, stock, side, q_in, N, n_nodes, key, perm[0]);
    for (int b = 0; b < passes; ++b) {
      hipLaunchKernelGGL(trades_hist_kernel, dim3((unsigned)tiles), dim3(64), 0, s, (const int32_t*)key, (const int32_t*)perm[cur], N, 8 * b,
                         hist, (int)tiles);
      if (int rc = pfo_iscan_launch(hist, 256 * tiles, base, scan, s)) return rc;
      hipLaunchKernelGGL(trades_scatter_kernel, dim3((unsigned)tiles), dim3(64), 0, s, (const int32_t*)key, (const int32_t*)perm[cur], N,
                         8 * b, (const int32_t*)base, (int)tiles, perm[cur ^ 1]);
      cur ^= 1;
    }
  }
  const unsigned grid = hold_grid(N * (int64_t)(64));      // one wavefront per sorted position, striding beyond the grid cap
  unsigned long long* ctr = reinterpret_cast<unsigned long long*>(counters);
#define TRADES_APPLY(NP, QTY)                                                                                                   \
  hipLaunchKernelGGL((trades_apply_kernel<NP, QTY>), dim3(grid), dim3(HOLD_BLOCK), 0, s, (const int32_t*)key, (const int32_t*)perm[cur], \
                     stock, side, q_in, ts, N, hold_idx, hold_len, hold_time, hold_qty, n_nodes, W, ctr)
  if (hold_qty) {
    if (W <= 64) TRADES_APPLY(1, true); else if (W <= 128) TRADES_APPLY(2, true); else TRADES_APPLY(4, true);
  } else {
    if (W <= 64) TRADES_APPLY(1, false); else if (W <= 128) TRADES_APPLY(2, false); else TRADES_APPLY(4, false);
  }
#undef TRADES_APPLY
  PFO_LAUNCH_CHECK();
  return PFO_OK;
}

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

// ------------------------------------------------------------------------------------------------ gather: position weights
// The weight rows of the position-weighted mean-variance order, aligned with pfo_holdings_gather's port_idx_out:
// one lane per slot of w_out[U, W], every slot written.  mode 0: the share count; mode 1: share count x last close (one rounded
// product; a stock outside the close table weighs 0.0, a stock never quoted NaN - the ranking kernel leaves both out).
namespace {
__global__ void __launch_bounds__(HOLD_BLOCK)
holdings_gather_weights_kernel(const int32_t* __restrict__ users, int64_t U, const int32_t* __restrict__ hold_idx,
                               const int32_t* __restrict__ hold_len, const double* __restrict__ hold_qty, int64_t n_nodes, int32_t W,
                               const double* __restrict__ last_close, int64_t n_stocks, int32_t mode, double* __restrict__ w_out) {
#pragma clang fp contract(off)
  const int64_t total = U * (int64_t)W, stride = (int64_t)gridDim.x * HOLD_BLOCK;
  for (int64_t i = (int64_t)blockIdx.x * HOLD_BLOCK + threadIdx.x; i < total; i += stride) {
    const int64_t q = i / W;
    const int32_t j = (int32_t)(i - q * W);
    const int64_t u = users[q];
    double w = 0.0;
    if (u >= 0 && u < n_nodes && j < std::min(std::max(hold_len[u], 0), W)) {
      w = hold_qty[u * W + j];
      if (mode == 1) {
        const int64_t s = hold_idx[u * W + j];
        w = (s >= 0 && s < n_stocks) ? w * last_close[s] : 0.0;
      }
    }
    w_out[i] = w;
  }
}
}  // namespace

extern "C" int pfo_holdings_gather_weights(const int32_t* users, int64_t U, const int32_t* hold_idx, const int32_t* hold_len,
                                           const double* hold_qty, int64_t n_nodes, int32_t W, const double* last_close, int64_t n_stocks,
                                           int32_t mode, double* w_out, void* stream) {
  PFO_REQUIRE(W >= 1 && W <= 256, "W must lie in [1, 256]");
  PFO_REQUIRE(U >= 0 && U <= INT64_MAX / 256, "U must not be negative");
  PFO_REQUIRE(n_nodes >= 1 && n_nodes < ((int64_t)1 << 31), "n_nodes must lie in [1, 2^31)");
  PFO_REQUIRE(n_stocks >= 0, "n_stocks must not be negative");
  PFO_REQUIRE(mode == 0 || mode == 1, "mode must be 0 (shares) or 1 (value)");
  if (U == 0) return PFO_OK;
  PFO_REQUIRE(users && hold_idx && hold_len && w_out, "null pointer");
  PFO_REQUIRE(hold_qty, "null hold_qty: the weights are share counts (a ledger with quantities)");
  PFO_REQUIRE(mode == 0 || last_close, "null last_close with mode 1 (value)");
  hipLaunchKernelGGL(holdings_gather_weights_kernel, dim3(hold_grid(U * (int64_t)W)), dim3(HOLD_BLOCK), 0, (hipStream_t)stream, users, U, hold_idx,
                     hold_len, hold_qty, n_nodes, W, last_close, n_stocks, mode, w_out);
  PFO_LAUNCH_CHECK();
  return PFO_OK;
}
