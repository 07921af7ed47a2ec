// Erasure by node (TGN.forget): expire's sibling.  A set of nodes leaves the served graph - a closed account, a delisted stock,
// an id taken in by mistake - and every table row of theirs returns to what add_nodes gives a new node.
//
//   gone u8[n_nodes], 1 = forgotten (pfo_nodes_flag builds it from a list of ids).  Entry i of row v is DROPPED iff gone[v] or
//   gone[adj_nbr[i]]; a neighbour id outside [0, n_nodes) counts as not gone.
//
// Unlike an expiry the survivors of a row are no suffix, and the rows are skewed (one hub item can hold a large share of all
// entries), so every pass here runs over ENTRIES, one lane each, never one thread per row:
//
//   pfo_csr_forget_plan : the keep decision per entry (its row by a binary search of indptr - a hub row costs what its entries
//                         cost) feeds the two-launch exclusive scan of scan64.hpp: new_pos[i] = the kept entries in front of
//                         entry i, new_pos[total] = the surviving total.  The kept count of row v is new_pos[indptr[v + 1]] -
//                         new_pos[indptr[v]], so its exclusive scan over rows is new_pos read at the row starts: one more launch
//                         over n_nodes + 1 rows writes new_indptr, with no second scan.
//   pfo_csr_forget_copy : entry i with keep[i] goes to new_pos[i]: reads coalesce, writes are monotone in the lane.
//   pfo_edge_rows_mark_nodes : pfo_edge_rows_mark's flags with "dropped" in place of "ts < cutoff"; pfo_edge_rows_plan /
//                         _compact and pfo_eidx_remap (ingest.hip) then run as they stand.
//   pfo_node_rows_reset : one launch over n_nodes rows; a wavefront reads 64 flags at once, the lane that owns a forgotten row
//                         writes its scalars, and the whole wavefront sweeps the row's vectors - consecutive lanes on
//                         consecutive dwords, no alignment assumed (a row of D floats starts anywhere when D % 4 != 0).
//
// All of it is bandwidth-bound and none of it is a step: a maintenance call with one read-back (the surviving total).
#include "common.hpp"
#include "scan64.hpp"
#include <algorithm>

namespace {

constexpr int FG_BLOCK = 256;
constexpr int64_t FG_MAX_GRID = 1 << 20;                   // beyond that the lanes stride
constexpr int32_t ROW_DROPPED = 1, ROW_SURVIVES = 2;       // pfo_edge_rows_mark's bits (ingest.hip: ROW_EXPIRED / ROW_SURVIVES)

unsigned fg_grid(int64_t total) { return (unsigned)std::min<int64_t>(std::max<int64_t>(1, pfo_ceil_div(total, FG_BLOCK)), FG_MAX_GRID); }

__global__ void __launch_bounds__(FG_BLOCK)
nodes_flag_kernel(const int32_t* __restrict__ ids, int64_t m, int64_t n_nodes, uint8_t* __restrict__ gone) {
  const int64_t stride = (int64_t)gridDim.x * FG_BLOCK;
  for (int64_t i = (int64_t)blockIdx.x * FG_BLOCK + threadIdx.x; i < m; i += stride) {
    const int64_t v = ids[i];
    if (v >= 1 && v < n_nodes) gone[v] = 1;                // (duplicates: every writer stores 1)
  }
}

// the row of flat position i: the last v with indptr[v] <= i - never an empty row, those share their successor's offset.
// Stays inside [0, n_nodes) whatever indptr holds.
__device__ __forceinline__ int64_t row_of_entry(const int64_t* __restrict__ indptr, int64_t n_nodes, int64_t i) {
  int64_t lo = 0, hi = n_nodes;                            // first v in [0, n_nodes] with indptr[v] > i
  while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (indptr[mid] <= i) lo = mid + 1; else hi = mid; }
  return lo > 0 ? lo - 1 : 0;
}
__device__ __forceinline__ bool entry_dropped(const int64_t* __restrict__ indptr, const int32_t* __restrict__ nbr, int64_t n_nodes,
                                              const uint8_t* __restrict__ gone, int64_t i) {
  const int64_t u = nbr[i];
  if (u >= 0 && u < n_nodes && gone[u]) return true;
  return gone[row_of_entry(indptr, n_nodes, i)] != 0;
}

struct ForgetKeep {                                        // the value scanned: 1 for an entry that stays
  const int64_t* indptr; const int32_t* nbr; int64_t n_nodes; const uint8_t* gone; uint8_t* keep;
  __device__ int64_t operator()(int64_t i) const {
    const uint8_t k = entry_dropped(indptr, nbr, n_nodes, gone, i) ? 0 : 1;
    keep[i] = k;
    return k;
  }
};
struct ForgetStore {
  int64_t* new_pos;
  __device__ void operator()(int64_t i, int64_t x) const { new_pos[i] = x; }     // (i == total: the surviving total)
};

__global__ void __launch_bounds__(FG_BLOCK)
forget_indptr_kernel(const int64_t* __restrict__ indptr, int64_t n_nodes, int64_t total, const int64_t* __restrict__ new_pos,
                     int64_t* __restrict__ new_indptr) {
  const int64_t stride = (int64_t)gridDim.x * FG_BLOCK;
  for (int64_t v = (int64_t)blockIdx.x * FG_BLOCK + threadIdx.x; v <= n_nodes; v += stride) {
    const int64_t p = indptr[v];
    new_indptr[v] = new_pos[p < 0 ? 0 : (p > total ? total : p)];
  }
}

__global__ void __launch_bounds__(FG_BLOCK)
forget_copy_kernel(const int32_t* __restrict__ onbr, const int32_t* __restrict__ oeid, const double* __restrict__ ots, int64_t old_total,
                   const uint8_t* __restrict__ keep, const int64_t* __restrict__ new_pos, int64_t total, int32_t* __restrict__ nnbr,
                   int32_t* __restrict__ neid, double* __restrict__ nts) {
  const int64_t stride = (int64_t)gridDim.x * FG_BLOCK;
  for (int64_t i = (int64_t)blockIdx.x * FG_BLOCK + threadIdx.x; i < old_total; i += stride) {
    if (!keep[i]) continue;
    const int64_t o = new_pos[i];
    if (o < 0 || o >= total) continue;                     // (a `total` that is not the plan's: write nothing outside the output)
    nnbr[o] = onbr[i]; neid[o] = oeid[i]; nts[o] = ots[i];
  }
}

__global__ void __launch_bounds__(FG_BLOCK)
edge_rows_mark_nodes_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ nbr, const int32_t* __restrict__ eidx,
                            int64_t n, int64_t n_nodes, const uint8_t* __restrict__ gone, int64_t n_rows, int32_t* __restrict__ flags) {
  const int64_t stride = (int64_t)gridDim.x * FG_BLOCK;
  for (int64_t i = (int64_t)blockIdx.x * FG_BLOCK + threadIdx.x; i < n; i += stride) {
    const int64_t r = eidx[i];
    if (r >= 0 && r < n_rows) atomicOr(&flags[r], entry_dropped(indptr, nbr, n_nodes, gone, i) ? ROW_DROPPED : ROW_SURVIVES);
  }
}

struct NodeTables {
  float* memory; int32_t D; float* last_update; float* msg_table; int32_t M; float* msg_time; uint8_t* has_msg;
  float* node_feat; int32_t Dn; int32_t* hold_idx; int32_t W; int32_t* hold_len; double* hold_time;
};

template <typename T>
__device__ __forceinline__ void fill_row(T* __restrict__ table, int64_t v, int32_t width, T value, int lane) {
  if (!table) return;
  T* row = table + v * (int64_t)width;
  for (int32_t j = lane; j < width; j += PFO_WAVE) row[j] = value;
}

// a wavefront per 64 consecutive rows
__global__ void __launch_bounds__(FG_BLOCK)
node_rows_reset_kernel(const uint8_t* __restrict__ gone, int64_t n_nodes, const NodeTables t) {
  const int lane = threadIdx.x & (PFO_WAVE - 1);
  const int64_t wave = ((int64_t)blockIdx.x * FG_BLOCK + threadIdx.x) / PFO_WAVE;
  const int64_t n_waves = (int64_t)gridDim.x * (FG_BLOCK / PFO_WAVE);
  for (int64_t base = wave * PFO_WAVE; base < n_nodes; base += n_waves * PFO_WAVE) {
    const int64_t v = base + lane;
    const bool mine = v < n_nodes && gone[v] != 0;
    if (mine) {                                            // the row's scalars: the lane that owns it
      if (t.last_update) t.last_update[v] = 0.0f;
      if (t.msg_time) t.msg_time[v] = 0.0f;
      if (t.has_msg) t.has_msg[v] = 0;
      if (t.hold_len) t.hold_len[v] = 0;
      if (t.hold_time) t.hold_time[v] = -__builtin_huge_val();
    }
    unsigned long long todo = __ballot(mine);              // the row's vectors: all 64 lanes, one forgotten row after the other
    while (todo) {
      const int64_t r = base + (__ffsll((long long)todo) - 1);
      todo &= todo - 1;
      fill_row(t.memory, r, t.D, 0.0f, lane);
      fill_row(t.msg_table, r, t.M, 0.0f, lane);
      fill_row(t.node_feat, r, t.Dn, 0.0f, lane);
      fill_row(t.hold_idx, r, t.W, (int32_t)-1, lane);
    }
  }
}

bool sizes_ok(int64_t n_nodes, int64_t total) { return n_nodes > 0 && n_nodes < ((int64_t)1 << 31) && total >= 0 && total < ((int64_t)1 << 31); }

}  // namespace

extern "C" int pfo_nodes_flag(const int32_t* ids, int64_t m, int64_t n_nodes, uint8_t* gone, void* stream) {
  PFO_REQUIRE(m >= 0 && n_nodes > 0 && n_nodes < ((int64_t)1 << 31), "bad sizes");
  PFO_REQUIRE(gone && (ids || m == 0), "null pointer");
  hipStream_t s = (hipStream_t)stream;
  PFO_REQUIRE(hipMemsetAsync(gone, 0, (size_t)n_nodes, s) == hipSuccess, "memset failed");
  if (m == 0) return PFO_OK;
  hipLaunchKernelGGL(nodes_flag_kernel, dim3(fg_grid(m)), dim3(FG_BLOCK), 0, s, ids, m, n_nodes, gone);
  PFO_LAUNCH_CHECK();
  return PFO_OK;
}

extern "C" int64_t pfo_csr_forget_scratch_bytes(int64_t n_nodes, int64_t total) {
  if (!sizes_ok(n_nodes, total)) return -1;
  return std::max<int64_t>(1, pfo_xs_tiles(total)) * 8;    // the tile totals of the scan over entries
}

extern "C" int pfo_csr_forget_plan(const int64_t* indptr, const int32_t* nbr, int64_t n_nodes, int64_t total, const uint8_t* gone,
                                   uint8_t* keep, int64_t* new_pos, int64_t* new_indptr, void* scratch, int64_t scratch_bytes,
                                   void* stream) {
  PFO_REQUIRE(sizes_ok(n_nodes, total), "bad sizes");
  PFO_REQUIRE(indptr && gone && new_pos && new_indptr && scratch && (total == 0 || (nbr && keep)), "null pointer");
  PFO_REQUIRE(scratch_bytes >= pfo_csr_forget_scratch_bytes(n_nodes, total), "short scratch");
  hipStream_t s = (hipStream_t)stream;
  if (total == 0) {                                        // an adjacency without entries: every offset is 0
    PFO_REQUIRE(hipMemsetAsync(new_indptr, 0, (size_t)(n_nodes + 1) * 8, s) == hipSuccess, "memset failed");
    PFO_REQUIRE(hipMemsetAsync(new_pos, 0, 8, s) == hipSuccess, "memset failed");
    return PFO_OK;
  }
  const unsigned nt = (unsigned)pfo_xs_tiles(total);
  int64_t* tile_sum = reinterpret_cast<int64_t*>(scratch);
  hipLaunchKernelGGL(xs_tile_kernel<ForgetKeep>, dim3(nt), dim3(XS_TILE), 0, s, (ForgetKeep{indptr, nbr, n_nodes, gone, keep}), total,
                     new_pos, tile_sum);
  hipLaunchKernelGGL(xs_offset_kernel<ForgetStore>, dim3(nt), dim3(XS_TILE), 0, s, (ForgetStore{new_pos}), total,
                     (const int64_t*)new_pos, (const int64_t*)tile_sum);
  hipLaunchKernelGGL(forget_indptr_kernel, dim3(fg_grid(n_nodes + 1)), dim3(FG_BLOCK), 0, s, indptr, n_nodes, total,
                     (const int64_t*)new_pos, new_indptr);
  PFO_LAUNCH_CHECK();
  return PFO_OK;
}

extern "C" int pfo_csr_forget_copy(const int32_t* old_nbr, const int32_t* old_eidx, const double* old_ts, int64_t old_total,
                                   const uint8_t* keep, const int64_t* new_pos, int64_t total, int32_t* new_nbr, int32_t* new_eidx,
                                   double* new_ts, void* stream) {
  PFO_REQUIRE(old_total >= 0 && old_total < ((int64_t)1 << 31) && total >= 0 && total <= old_total, "bad sizes");
  if (total == 0) return PFO_OK;
  PFO_REQUIRE(old_nbr && old_eidx && old_ts && keep && new_pos && new_nbr && new_eidx && new_ts, "null pointer");
  hipLaunchKernelGGL(forget_copy_kernel, dim3(fg_grid(old_total)), dim3(FG_BLOCK), 0, (hipStream_t)stream, old_nbr, old_eidx, old_ts,
                     old_total, keep, new_pos, total, new_nbr, new_eidx, new_ts);
  PFO_LAUNCH_CHECK();
  return PFO_OK;
}

extern "C" int pfo_edge_rows_mark_nodes(const int64_t* indptr, const int32_t* nbr, const int32_t* eidx, int64_t n, int64_t n_nodes,
                                        const uint8_t* gone, int64_t n_rows, int32_t* flags, void* stream) {
  PFO_REQUIRE(sizes_ok(n_nodes, n) && n_rows >= 1 && n_rows < ((int64_t)1 << 31), "bad sizes");
  if (n == 0) return PFO_OK;
  PFO_REQUIRE(indptr && nbr && eidx && gone && flags, "null pointer");
  hipLaunchKernelGGL(edge_rows_mark_nodes_kernel, dim3(fg_grid(n)), dim3(FG_BLOCK), 0, (hipStream_t)stream, indptr, nbr, eidx, n, n_nodes,
                     gone, n_rows, flags);
  PFO_LAUNCH_CHECK();
  return PFO_OK;
}

extern "C" int pfo_node_rows_reset(const uint8_t* gone, int64_t n_nodes, float* memory, int32_t D, float* last_update, float* msg_table,
                                   int32_t M, float* msg_time, uint8_t* has_msg, float* node_feat, int32_t Dn, int32_t* hold_idx,
                                   int32_t W, int32_t* hold_len, double* hold_time, void* stream) {
  PFO_REQUIRE(n_nodes > 0 && n_nodes < ((int64_t)1 << 31), "bad sizes");
  PFO_REQUIRE((!memory || D >= 1) && (!msg_table || M >= 1) && (!node_feat || Dn >= 1) && (!hold_idx || W >= 1), "a table without columns");
  PFO_REQUIRE(gone, "null pointer");
  const NodeTables t{memory, D, last_update, msg_table, M, msg_time, has_msg, node_feat, Dn, hold_idx, W, hold_len, hold_time};
  hipLaunchKernelGGL(node_rows_reset_kernel, dim3(fg_grid(n_nodes)), dim3(FG_BLOCK), 0, (hipStream_t)stream, gone, n_nodes, t);
  PFO_LAUNCH_CHECK();
  return PFO_OK;
}
