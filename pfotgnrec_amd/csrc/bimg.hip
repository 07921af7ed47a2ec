// The image builders: a weight operand pre-split into the LDS image the image kernels (gemm_bx.hip, gemm_fused.hip) read.
#include "gemm_dev.hpp"
#include <algorithm>

// Pre-split image of a weight operand for the image kernels: [k-tile][piece][row n, padded to BN][64 B],
// the exact LDS image of those kernels (same swizzle), zero-padded in n and k.  W(n, k) = src[n*ld + k] or, with
// `trans`, src[k*ld + n] - so a k-major ("NN") operand becomes a row-major one for free.
struct BimgDev {
  const float* src[PFO_BIMG_MAX]; int64_t ld[PFO_BIMG_MAX]; int N[PFO_BIMG_MAX], K[PFO_BIMG_MAX], trans[PFO_BIMG_MAX];
  void* dst[PFO_BIMG_MAX]; int rows[PFO_BIMG_MAX];      // rows: image rows this problem fills (incl. zero padding)
  int row0[PFO_BIMG_MAX], rows_total[PFO_BIMG_MAX];     // first image row of the problem, padded rows of the whole image
  int gate[PFO_BIMG_MAX], gate_D[PFO_BIMG_MAX];         // GRU gate-ordered image (gemm.hpp PfoBimg::gate): 0 = plain
};
// Source row of image row n of a GRU gate-ordered image (gru_fused_kernel): blocks of GF_BN = 128 image rows = two groups of
// four 16-row tiles (r, z, n_i, n_h) for 16 hidden units each.  gate 1: the message weights W_ih [3D, M] (no n_h rows),
// gate 2: the hidden-state weights W_hh [3D, D] (no n_i rows).  -1: a zero row.
__device__ __forceinline__ int bimg_gate_row(int n, int which, int D) {
  const int b = n >> 7, t = (n & 127) >> 4, i = n & 15;
  const int u = 32 * b + 16 * (t >> 2) + i, gt = t & 3;
  if (u >= D) return -1;
  if (gt == 0) return u;
  if (gt == 1) return D + u;
  if (gt == 2) return which == 1 ? 2 * D + u : -1;
  return which == 2 ? 2 * D + u : -1;
}
// The fp16x2 image (FMT 1): [k-tile][piece h | l][row][64 B] in the same swizzled layout, then one int32 per image row: the
// biased exponent E of the row's largest magnitude (clamped); the row is stored times 2^(HX_TOP - E).
__device__ __forceinline__ int bimg_src_row(const BimgDev& g, int z, int n) {
  if (g.gate[z]) return bimg_gate_row(n, g.gate[z], g.gate_D[z]);
  return n < g.N[z] ? n : -1;
}
__device__ __forceinline__ int32_t* bimg_exps(const BimgDev& g, int z) {
  const int T = (g.K[z] + 31) / 32;
  return reinterpret_cast<int32_t*>(reinterpret_cast<char*>(g.dst[z]) + (int64_t)T * 2 * g.rows_total[z] * 64);
}
// Row-major operands (and the GRU's gate-ordered ones): one wavefront per image row, lanes along k with 16-byte loads; the
// first pass finds the row maximum, the second (L1 / L2 hits) converts.  vec: every row start and K are multiples of 4 floats.
__global__ __launch_bounds__(256) void bimg_h_rows_kernel(const BimgDev g) {
  const int z = blockIdx.y;
  const int K = g.K[z], rows = g.rows[z];
  const int T = (K + 31) / 32;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= rows) return;
  const int lane = threadIdx.x & 63;
  const int sr = bimg_src_row(g, z, n);
  const float* __restrict__ row = g.src[z] + (int64_t)max(sr, 0) * g.ld[z];
  const bool vec = ((g.ld[z] | K) & 3) == 0 && (((uintptr_t)g.src[z]) & 15) == 0;
  auto ld4k = [&](int k) -> float4 {                            // k % 4 == 0
    if (sr < 0 || k >= K) return float4{0.f, 0.f, 0.f, 0.f};
    if (vec) return *reinterpret_cast<const float4*>(row + k);
    return float4{row[k], k + 1 < K ? row[k + 1] : 0.f, k + 2 < K ? row[k + 2] : 0.f, k + 3 < K ? row[k + 3] : 0.f};
  };
  float m = 0.f;
  for (int ci = lane; ci < 4 * T; ci += 64) m = fmaxf(m, hx_absmax8(ld4k(8 * ci), ld4k(8 * ci + 4)));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  const int E = hx_exp_of(m);
  const int se = HX_TOP - E;
  char* dst = reinterpret_cast<char*>(g.dst[z]);
  const int ng = n + g.row0[z];
  const int64_t piece = (int64_t)g.rows_total[z] * 64;
  for (int ci = lane; ci < 4 * T; ci += 64) {
    const int t = ci >> 2, c = ci & 3;
    uint2 h0, l0, h1, l1;
    hx_split4(ld4k(8 * ci), se, h0, l0);
    hx_split4(ld4k(8 * ci + 4), se, h1, l1);
    const int64_t off = (int64_t)ng * 64 + ((c ^ bx_swz(ng)) << 4);
    *reinterpret_cast<uint4*>(dst + ((int64_t)t * 2 + 0) * piece + off) = uint4{h0.x, h0.y, h1.x, h1.y};
    *reinterpret_cast<uint4*>(dst + ((int64_t)t * 2 + 1) * piece + off) = uint4{l0.x, l0.y, l1.x, l1.y};
  }
  if (lane == 0) bimg_exps(g, z)[ng] = E;
}
// Lists with k-major ("trans") operands take two launches: the row exponents (one wavefront per image row; a k-major row is
// a strided column of the source, its 64-byte lines shared with the neighbouring rows' wavefronts), then the conversion in
// one thread per (tile, row, 16-byte chunk), coalesced along n for k-major sources.
__global__ __launch_bounds__(256) void bimg_exp_kernel(const BimgDev g) {
  const int z = blockIdx.y;
  const int K = g.K[z], rows = g.rows[z];
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= rows) return;
  const int lane = threadIdx.x & 63;
  const int sr = bimg_src_row(g, z, n);
  const float* __restrict__ src = g.src[z];
  const int64_t ld = g.ld[z];
  float m = 0.f;
  if (sr >= 0) {
    if (g.trans[z]) for (int k = lane; k < K; k += 64) m = fmaxf(m, fabsf(src[(int64_t)k * ld + sr]));
    else for (int k = lane; k < K; k += 64) m = fmaxf(m, fabsf(src[(int64_t)sr * ld + k]));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if (lane == 0) bimg_exps(g, z)[n + g.row0[z]] = hx_exp_of(m);
}
__global__ __launch_bounds__(256) void bimg_h_kernel(const BimgDev g) {
  const int z = blockIdx.y;
  const int N = g.N[z], K = g.K[z], rows = g.rows[z];
  const int T = (K + 31) / 32;
  const int64_t total = (int64_t)T * rows * 4;                 // one thread per (tile, row, 16-byte chunk)
  const float* __restrict__ src = g.src[z];
  const int64_t ld = g.ld[z];
  char* dst = reinterpret_cast<char*>(g.dst[z]);
  const int32_t* exps = bimg_exps(g, z);
  const int64_t piece = (int64_t)g.rows_total[z] * 64;
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    int t, n, c;
    if (g.trans[z]) { n = (int)(i % rows); c = (int)((i / rows) & 3); t = (int)(i / (4 * (int64_t)rows)); }
    else            { c = (int)(i & 3); n = (int)((i >> 2) % rows); t = (int)((i >> 2) / rows); }
    const int sr = bimg_src_row(g, z, n);
    float x[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int k = 32 * t + 8 * c + e;
      x[e] = (sr >= 0 && k < K) ? (g.trans[z] ? src[(int64_t)k * ld + sr] : src[(int64_t)sr * ld + k]) : 0.f;
    }
    const int ng = n + g.row0[z];
    const int se = HX_TOP - exps[ng];
    uint2 h0, l0, h1, l1;
    hx_split4(float4{x[0], x[1], x[2], x[3]}, se, h0, l0);
    hx_split4(float4{x[4], x[5], x[6], x[7]}, se, h1, l1);
    const int64_t off = (int64_t)ng * 64 + ((c ^ bx_swz(ng)) << 4);
    *reinterpret_cast<uint4*>(dst + ((int64_t)t * 2 + 0) * piece + off) = uint4{h0.x, h0.y, h1.x, h1.y};
    *reinterpret_cast<uint4*>(dst + ((int64_t)t * 2 + 1) * piece + off) = uint4{l0.x, l0.y, l1.x, l1.y};
  }
}

int64_t pfo_bimg_bytes(int N, int K) { return (int64_t)pfo_ceil_div(K, 32) * 3 * pfo_align_up(N, BN) * 64; }

int pfo_bimg_launch(const PfoBimg* list, int n, hipStream_t stream) {
  PFO_REQUIRE(n >= 1 && n <= PFO_BIMG_MAX, "bad image count");
  BimgDev d;
  int64_t most = 0;
  for (int i = 0; i < n; ++i) {
    PFO_REQUIRE(list[i].src && list[i].dst && list[i].N > 0 && list[i].K > 0, "bad image problem");
    PFO_REQUIRE((((uintptr_t)list[i].dst) & 15) == 0, "image must be 16-byte aligned");
    d.src[i] = list[i].src; d.ld[i] = list[i].ld; d.N[i] = list[i].N; d.K[i] = list[i].K; d.trans[i] = list[i].trans;
    d.dst[i] = list[i].dst;
    d.row0[i] = list[i].row0;
    d.gate[i] = list[i].gate; d.gate_D[i] = list[i].gate_D;
    if (list[i].gate) {
      // gate-ordered: the image has pfo_gru_img_rows(D) rows, all written by this problem (zero rows included); N = 3 D source rows
      PFO_REQUIRE(list[i].gate_D > 0 && list[i].N == 3 * list[i].gate_D && !list[i].trans && list[i].rows_total == 0, "bad gate-ordered image");
      d.rows_total[i] = d.rows[i] = pfo_gru_img_rows(list[i].gate_D);
      most = std::max<int64_t>(most, (int64_t)pfo_ceil_div(list[i].K, 32) * d.rows[i] * 4);
      continue;
    }
    d.rows_total[i] = list[i].rows_total > 0 ? (int)pfo_align_up(list[i].rows_total, BN) : (int)pfo_align_up(list[i].N, BN);
    // rows this problem writes: a plain image and the last operand of a stack include the zero padding up to the padded end
    d.rows[i] = list[i].rows_total > 0 ? (list[i].last ? d.rows_total[i] - d.row0[i] : list[i].N) : d.rows_total[i];
    PFO_REQUIRE(d.row0[i] >= 0 && d.rows[i] >= list[i].N && d.row0[i] + d.rows[i] <= d.rows_total[i], "bad stacked image rows");
    most = std::max<int64_t>(most, (int64_t)pfo_ceil_div(list[i].K, 32) * d.rows[i] * 4);
  }
  int most_rows = 0;
  bool any_trans = false;
  for (int i = 0; i < n; ++i) { most_rows = std::max(most_rows, d.rows[i]); any_trans = any_trans || d.trans[i] != 0; }
  if (!any_trans) PFO_KLAUNCH(bimg_h_rows_kernel, dim3((unsigned)pfo_ceil_div(most_rows, 4), n), dim3(256), 0, stream, d);
  else {
    PFO_KLAUNCH(bimg_exp_kernel, dim3((unsigned)pfo_ceil_div(most_rows, 4), n), dim3(256), 0, stream, d);
    PFO_KLAUNCH(bimg_h_kernel, dim3((unsigned)pfo_ceil_div(most, 256), n), dim3(256), 0, stream, d);
  }
  PFO_LAUNCH_CHECK();
  return PFO_OK;
}
