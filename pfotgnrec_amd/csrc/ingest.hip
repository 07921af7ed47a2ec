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
#include "common.hpp"
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
