// Serving ingest: rows of RAW edge features are z-scored with the model's FROZEN column statistics and written behind the live
// rows of the edge-feature table (TGN.add_edge_features / TGN.ingest).
//
// The arithmetic is numpy's `ef -= mean; ef /= std` on fp32 arrays (the constructor's normalisation, tgn.py
// _normalise_edge_features): ONE correctly rounded subtraction, then ONE correctly rounded division, so that a row appended
// later holds the very bits it would hold had it been in the table the statistics were taken from.  __fsub_rn / __fdiv_rn are
// the round-to-nearest-even forms that the compiler neither contracts into an FMA nor replaces by a reciprocal multiply
// (build.py compiles with -O3 and the HIP default -ffp-contract=fast; a subtraction feeding a division has no fused form, and
// fp32 division is the correctly rounded v_div_scale / v_div_fmas / v_div_fixup sequence unless a fast-math flag asks
// otherwise - build.py passes none - but the intrinsics say it where it matters).  fp32 denormals are kept on gfx950 (HIP does
// not flush them unless asked to), as numpy keeps them.  A zero-variance column gives x/0 = +-inf and 0/0 = NaN like numpy.
//
// Layout: one lane per ELEMENT of the [m, Ef] block, consecutive lanes on consecutive addresses (rows are contiguous, so the
// block is one contiguous range of the table): loads and stores coalesce for every Ef and every row0, with no alignment
// assumption - row0 * Ef is no multiple of 4 in general.  The column statistics (Ef floats) come from the cache.  A serving
// tick is a few KB: the kernel is bandwidth-trivial and a single launch; it is not tuned.
//
// Retention (TGN.expire): the way back.  Rows of the table that only EXPIRED adjacency entries name are released, the others
// move down in order (pfo_edge_rows_mark / _plan / _compact), and the adjacency's edge indices follow (pfo_eidx_remap).  The
// table is shared between finders, so the flags are gathered over every finder taking part before anything moves.
#include "common.hpp"
#include "scan64.hpp"
#include <algorithm>

namespace {

constexpr int INGEST_BLOCK = 256;
constexpr int64_t INGEST_MAX_GRID = 1 << 20;     // beyond that the lanes stride (2^28 elements per sweep)

__global__ void __launch_bounds__(INGEST_BLOCK)
edge_rows_append_kernel(const float* __restrict__ raw, const float* __restrict__ mean, const float* __restrict__ stdv,
                        int64_t total, int32_t Ef, float* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * INGEST_BLOCK;
  for (int64_t i = (int64_t)blockIdx.x * INGEST_BLOCK + threadIdx.x; i < total; i += stride) {
    const int j = (int)(i % Ef);
    out[i] = __fdiv_rn(__fsub_rn(raw[i], mean[j]), stdv[j]);
  }
}

// ---- retention
constexpr int32_t ROW_EXPIRED = 1, ROW_SURVIVES = 2;       // bits of flags[r]: some expired / some surviving entry names row r

__global__ void __launch_bounds__(INGEST_BLOCK)
edge_rows_mark_kernel(const int32_t* __restrict__ eidx, const double* __restrict__ ts, int64_t n, double cutoff, int64_t n_rows,
                      int32_t* __restrict__ flags) {
  const int64_t stride = (int64_t)gridDim.x * INGEST_BLOCK;
  for (int64_t i = (int64_t)blockIdx.x * INGEST_BLOCK + threadIdx.x; i < n; i += stride) {
    const int64_t r = eidx[i];
    if (r >= 0 && r < n_rows) atomicOr(&flags[r], ts[i] < cutoff ? ROW_EXPIRED : ROW_SURVIVES);   // (an edge has two entries: no contention to speak of)
  }
}

// released <=> r >= 1, an expired entry names r and no surviving one does; rows nobody names stay
__device__ __forceinline__ bool row_kept(const int32_t* flags, int64_t r) { return r == 0 || flags[r] != ROW_EXPIRED; }
struct RowKeep {
  const int32_t* flags;
  __device__ int64_t operator()(int64_t r) const { return row_kept(flags, r) ? 1 : 0; }
};
struct RowRemap {
  const int32_t* flags; int32_t* remap; int32_t* n_keep; int64_t n_rows;
  __device__ void operator()(int64_t r, int64_t x) const {
    if (r == n_rows) *n_keep = (int32_t)x;
    else remap[r] = row_kept(flags, r) ? (int32_t)x : -1;
  }
};

// kept rows into a TEMPORARY, densely: a row moves DOWN inside the table's own storage, where source and destination ranges
// of different rows overlap - the copy back (stream-ordered behind this launch) is the only writer of the table
__global__ void __launch_bounds__(INGEST_BLOCK)
edge_rows_gather_kernel(const float* __restrict__ table, const int32_t* __restrict__ remap, int64_t total, int32_t Ef, int64_t n_keep,
                        float* __restrict__ tmp) {
  const int64_t stride = (int64_t)gridDim.x * INGEST_BLOCK;
  for (int64_t i = (int64_t)blockIdx.x * INGEST_BLOCK + threadIdx.x; i < total; i += stride) {
    const int64_t r = i / Ef;
    const int64_t d = remap[r];
    if (d >= 0 && d < n_keep) tmp[d * Ef + (i - r * Ef)] = table[i];
  }
}

// element-wise and in place: every lane reads and writes its own entry
__global__ void __launch_bounds__(INGEST_BLOCK)
eidx_remap_kernel(int32_t* __restrict__ eidx, int64_t n, const int32_t* __restrict__ remap, int64_t n_rows) {
  const int64_t stride = (int64_t)gridDim.x * INGEST_BLOCK;
  for (int64_t i = (int64_t)blockIdx.x * INGEST_BLOCK + threadIdx.x; i < n; i += stride) {
    const int64_t r = eidx[i];
    if (r < 0 || r >= n_rows) continue;
    const int32_t d = remap[r];
    if (d >= 0) eidx[i] = d;                  // (a surviving entry never names a released row: its flag kept the row)
  }
}

unsigned ingest_grid(int64_t total) { return (unsigned)std::min<int64_t>(pfo_ceil_div(total, INGEST_BLOCK), INGEST_MAX_GRID); }

}  // namespace

extern "C" int pfo_edge_rows_append(const float* raw, const float* mean, const float* stdv, int64_t m, int32_t Ef, float* table,
                                    int64_t row0, int64_t cap, void* stream) {
  PFO_REQUIRE(m >= 0, "m must not be negative");
  PFO_REQUIRE(Ef >= 1, "Ef must be at least 1");
  PFO_REQUIRE(row0 >= 0 && cap >= 0 && row0 <= cap, "row0 must lie in [0, cap]");
  PFO_REQUIRE(m <= cap - row0, "the rows do not fit: row0 + m > cap (grow the table first)");
  PFO_REQUIRE(cap <= INT64_MAX / Ef, "cap * Ef overflows");
  if (m == 0) return PFO_OK;
  PFO_REQUIRE(raw && mean && stdv && table, "null pointer");
  const int64_t total = m * (int64_t)Ef;
  const int64_t grid = std::min<int64_t>(pfo_ceil_div(total, INGEST_BLOCK), INGEST_MAX_GRID);
  hipLaunchKernelGGL(edge_rows_append_kernel, dim3((unsigned)grid), dim3(INGEST_BLOCK), 0, (hipStream_t)stream, raw, mean, stdv,
                     total, Ef, table + row0 * (int64_t)Ef);
  PFO_LAUNCH_CHECK();
  return PFO_OK;
}

extern "C" int pfo_edge_rows_mark(const int32_t* eidx, const double* ts, int64_t n, double cutoff, int64_t n_rows, int32_t* flags,
                                  void* stream) {
  PFO_REQUIRE(n >= 0 && n_rows >= 1 && n_rows < ((int64_t)1 << 31), "bad sizes");
  PFO_REQUIRE(cutoff == cutoff && cutoff - cutoff == 0.0, "the cutoff must be finite");
  if (n == 0) return PFO_OK;
  PFO_REQUIRE(eidx && ts && flags, "null pointer");
  hipLaunchKernelGGL(edge_rows_mark_kernel, dim3(ingest_grid(n)), dim3(INGEST_BLOCK), 0, (hipStream_t)stream, eidx, ts, n, cutoff,
                     n_rows, flags);
  PFO_LAUNCH_CHECK();
  return PFO_OK;
}

extern "C" int64_t pfo_edge_rows_plan_scratch_bytes(int64_t n_rows) {
  if (n_rows < 1 || n_rows >= ((int64_t)1 << 31)) return -1;
  return (n_rows + pfo_xs_tiles(n_rows)) * 8;
}

extern "C" int pfo_edge_rows_plan(const int32_t* flags, int64_t n_rows, int32_t* remap, int32_t* n_keep, void* scratch,
                                  int64_t scratch_bytes, void* stream) {
  PFO_REQUIRE(n_rows >= 1 && n_rows < ((int64_t)1 << 31), "bad row count");
  PFO_REQUIRE(flags && remap && n_keep && scratch, "null pointer");
  PFO_REQUIRE(scratch_bytes >= pfo_edge_rows_plan_scratch_bytes(n_rows), "short scratch");
  hipStream_t s = (hipStream_t)stream;
  const unsigned nt = (unsigned)pfo_xs_tiles(n_rows);
  int64_t* local = reinterpret_cast<int64_t*>(scratch);
  int64_t* tile_sum = local + n_rows;
  hipLaunchKernelGGL(xs_tile_kernel<RowKeep>, dim3(nt), dim3(XS_TILE), 0, s, (RowKeep{flags}), n_rows, local, tile_sum);
  hipLaunchKernelGGL(xs_offset_kernel<RowRemap>, dim3(nt), dim3(XS_TILE), 0, s, (RowRemap{flags, remap, n_keep, n_rows}), n_rows,
                     (const int64_t*)local, (const int64_t*)tile_sum);
  PFO_LAUNCH_CHECK();
  return PFO_OK;
}

extern "C" int pfo_edge_rows_compact(float* table, int64_t n_rows, int64_t n_keep, int32_t Ef, const int32_t* remap, float* tmp,
                                     void* stream) {
  PFO_REQUIRE(Ef >= 1, "Ef must be at least 1");
  PFO_REQUIRE(n_rows >= 1 && n_keep >= 1 && n_keep <= n_rows, "n_keep must lie in [1, n_rows]");
  PFO_REQUIRE(n_rows <= INT64_MAX / 4 / Ef, "n_rows * Ef overflows");
  if (n_keep == n_rows) return PFO_OK;                       // nothing released: the identity map, nothing moves
  PFO_REQUIRE(table && remap && tmp, "null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int64_t total = n_rows * (int64_t)Ef, kept = n_keep * (int64_t)Ef;
  hipLaunchKernelGGL(edge_rows_gather_kernel, dim3(ingest_grid(total)), dim3(INGEST_BLOCK), 0, s, (const float*)table, remap, total,
                     Ef, n_keep, tmp);
  PFO_LAUNCH_CHECK();
  PFO_REQUIRE(hipMemcpyAsync(table, tmp, (size_t)kept * 4, hipMemcpyDeviceToDevice, s) == hipSuccess, "copy back failed");
  PFO_REQUIRE(hipMemsetAsync(table + kept, 0, (size_t)(total - kept) * 4, s) == hipSuccess, "memset failed");   // rows behind the live count are zero
  return PFO_OK;
}

extern "C" int pfo_eidx_remap(int32_t* eidx, int64_t n, const int32_t* remap, int64_t n_rows, void* stream) {
  PFO_REQUIRE(n >= 0 && n_rows >= 1, "bad sizes");
  if (n == 0) return PFO_OK;
  PFO_REQUIRE(eidx && remap, "null pointer");
  hipLaunchKernelGGL(eidx_remap_kernel, dim3(ingest_grid(n)), dim3(INGEST_BLOCK), 0, (hipStream_t)stream, eidx, n, remap, n_rows);
  PFO_LAUNCH_CHECK();
  return PFO_OK;
}
