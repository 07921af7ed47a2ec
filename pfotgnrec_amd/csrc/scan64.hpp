// Exclusive scan of n int64 values in two launches, shared by the retention kernels (csr.hip pfo_csr_expire_plan, ingest.hip
// pfo_edge_rows_plan) and the erasure by node (forget.hip pfo_csr_forget_plan, over entries).  The values are PRODUCED by a functor and the scanned offsets are CONSUMED by one, so the pass that
// makes the counts and the pass that uses the offsets need no launch of their own:
//
//   xs_tile_kernel   : one workgroup per tile of XS_TILE values; v = f(i); local[i] = exclusive sum inside the tile (wave scan
//                      by shuffles over XS_WAVE lanes, then the XS_TILE / XS_WAVE wave totals through LDS); tile_sum[b] = the
//                      tile's total.
//   xs_offset_kernel : tile b sums tile_sum[0, b) itself - XS_TILE lanes stride over the earlier tiles, so a tile index above
//                      XS_TILE (more than XS_TILE^2 = 1,048,576 values) gives a lane more than one term - and hands
//                      g(i, local[i] + offset) every value; the last tile also hands over g(n, total).
//
// Nothing waits on another workgroup inside a launch (no look-back): the kernel boundary is the only hand-off.  Tile b reads b
// sums: quadratic in n / 1024, 50 M cached reads at ten million values - a maintenance call, not a step.
#pragma once
#include "common.hpp"

#define XS_WAVE 64
#define XS_TILE 1024

static inline int64_t pfo_xs_tiles(int64_t n) { return pfo_ceil_div(n, XS_TILE); }

#ifdef __HIPCC__
template <typename F>
__global__ __launch_bounds__(XS_TILE) void xs_tile_kernel(F f, int64_t n, int64_t* __restrict__ local, int64_t* __restrict__ tile_sum) {
  __shared__ int64_t s_w[XS_TILE / XS_WAVE];
  const int64_t i = (int64_t)blockIdx.x * XS_TILE + threadIdx.x;
  const int lane = threadIdx.x & (XS_WAVE - 1), wave = threadIdx.x / XS_WAVE;
  const int64_t v = i < n ? f(i) : 0;
  int64_t incl = v;
#pragma unroll
  for (int o = 1; o < XS_WAVE; o <<= 1) {
    const int64_t u = __shfl_up(incl, o, XS_WAVE);
    if (lane >= o) incl += u;
  }
  if (lane == XS_WAVE - 1) s_w[wave] = incl;
  __syncthreads();
  int64_t woff = 0;
  for (int w = 0; w < wave; ++w) woff += s_w[w];
  if (i < n) local[i] = woff + incl - v;
  if (threadIdx.x == XS_TILE - 1) tile_sum[blockIdx.x] = woff + incl;
}

template <typename G>
__global__ __launch_bounds__(XS_TILE) void xs_offset_kernel(G g, int64_t n, const int64_t* local,      // (g may store into `local`)
                                                            const int64_t* __restrict__ tile_sum) {
  __shared__ int64_t s_w[XS_TILE / XS_WAVE];
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x & (XS_WAVE - 1), wave = threadIdx.x / XS_WAVE;
  int64_t part = 0;
  for (int64_t t = threadIdx.x; t < b; t += XS_TILE) part += tile_sum[t];
#pragma unroll
  for (int o = XS_WAVE / 2; o > 0; o >>= 1) part += __shfl_xor(part, o, XS_WAVE);
  if (lane == 0) s_w[wave] = part;
  __syncthreads();
  int64_t off = 0;
  for (int w = 0; w < XS_TILE / XS_WAVE; ++w) off += s_w[w];
  const int64_t i = b * XS_TILE + threadIdx.x;
  if (i < n) g(i, local[i] + off);
  if (b == (int64_t)gridDim.x - 1 && threadIdx.x == 0) g(n, off + tile_sum[b]);
}
#endif  // __HIPCC__
