// fp32 contraction on the gfx950 matrix cores: v_mfma_f32_16x16x4_f32 (exact fp32, 256 FLOP/clk/CU).
//
// Why fp32 MFMA: the parity bar is 1e-4 relative on embeddings (BASELINE.json north_star), which
// rules out bf16/fp16 operands; gfx950 has no xf32.  Tile = 128 x 176 x 32, 4 wavefronts, each
// wavefront owning a 32 x 176 strip as 2 x 11 MFMA tiles (88 accumulator VGPRs).  176 = 11*16 is
// chosen for THIS model: every N it sees (D=172, 2D=344, 2D+Ef=348, 3D=516) is k*176 minus a few
// columns, so column padding waste is ~2% where a 128/256-wide tile would waste 10-25%.
// Operands are staged global -> registers -> LDS (one LDS buffer, next tile's global loads in
// flight during the MFMAs of the current one); LDS row strides (34 / 144 / 176 floats) make every
// fragment read conflict-free for the two 32-lane halves of ds_read_b32.
//
// This file: the exact-fp32 tile (gemm_tile) and its three users - the plain kernel, the multi-problem launch and the grouped
// weight gradient of operands that admit no float4 loads - and the two fp32 folds beside them (rank-1 updates, slab sums).
#include "gemm_dev.hpp"
#include <algorithm>

constexpr int LDA_RM = 34;      // row-major A/B tile row stride (floats): 34 mod 32 = 2 -> banks 2r+g distinct
constexpr int LDA_KM = 144;     // k-major A tile row stride: 144 mod 32 = 16
constexpr int LDB_KM = 176;     // k-major B tile row stride: 176 mod 32 = 16
constexpr int AS_FLOATS = 4608;   // max(128*34, 32*144)
constexpr int BS_FLOATS = 5984;   // max(176*34, 32*176)

// Two workgroup shapes, both 256 threads = 4 wavefronts:
//   BIG   : 128 x 176 output tile, wavefront w owns rows [32w, 32w+32) x all 11 column tiles   (2 x 11 MFMA tiles)
//   SMALL :  32 x 176 output tile, wavefront w owns all 32 rows x column tiles {w, w+4, w+8}    (2 x 3 MFMA tiles)
// SMALL exists for the layer-2 launches (M = 2560 rows): 4x the workgroups, so the chip is not left idle.
// The K loop runs over a flattened list of 32-deep tiles of up to two K-concatenated sources; the global loads of
// tile t+1 are in flight (registers) while the MFMAs of tile t run from LDS.
template <bool A_KM, bool B_KM, int TILE, bool VEC>
__device__ __forceinline__ void gemm_tile(const GemmDev& p, const int bx, const int by, int zb, const int split_in,
                                          float* __restrict__ lds_a, float* __restrict__ lds_b) {
  constexpr bool TINY = (TILE == 2);           // 32 x 64 tile: the multi-problem launches (see gemm_multi_kernel)
  constexpr bool SMALL = (TILE == 1) || TINY;
  constexpr int TBM = SMALL ? 32 : BM;
  constexpr int TBN = TINY ? 64 : BN;          // columns of the tile
  constexpr int NB4 = TBN / 4;                 // float4 per k-row of a k-major B tile
  constexpr int NBL = (TBN * 8 + 255) / 256;   // float4 of the B tile per thread
  constexpr int NJ = TINY ? 1 : (SMALL ? 3 : 11);
  constexpr int NI = 2;                        // 16-row strips per wavefront
  constexpr int NA = TBM / 32;                 // float4 per thread for the A tile
  constexpr int LDAK = TINY ? 48 : LDA_KM;     // k-major A row stride, = 16 mod 32
  constexpr int LDBK = TINY ? 80 : LDB_KM;     // k-major B row stride, = 16 mod 32
  float* const As[1] = {lds_a};
  float* const Bs[1] = {lds_b};
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int m0 = bx * TBM, n0 = by * TBN;
  const int split = split_in;

  int Mlim = p.M;
  int Kext0 = p.K[0];
  if (p.m_dev) {
    const int md = *p.m_dev;
    if (A_KM) Kext0 = min(Kext0, md); else Mlim = min(Mlim, md);
  }
  if (!A_KM && m0 >= Mlim) return;
  int kbeg = 0, kend0 = Kext0;
  if (A_KM && p.nsplit > 1) {
    // with a device-side K bound (GRU rows) the chunks are cut from the ACTUAL extent so every split has work
    const int chunk = p.dyn_chunk ? ((Kext0 + p.nsplit - 1) / p.nsplit + BK - 1) / BK * BK : p.split_chunk;
    kbeg = split * chunk;
    kend0 = min(Kext0, kbeg + chunk);
  }
  const int wrow = SMALL ? 0 : 32 * wave;      // first tile row of this wavefront
  const int wcol = SMALL ? 16 * wave : 0;      // first tile column; SMALL strides columns by 64

  f32x4 acc[NI][NJ];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // flattened tile list
  const int T0 = kend0 > kbeg ? (kend0 - kbeg + BK - 1) / BK : 0;
  const int T1 = (p.K[1] > 0 && p.A[1]) ? (p.K[1] + BK - 1) / BK : 0;
  const int T = T0 + T1;

  float4 a_reg[NA], b_reg[NBL];
  float4 a_reg2[TINY ? NA : 1], b_reg2[TINY ? NBL : 1];   // TINY: second staging set (loads two tiles ahead)
  const float* a_row[NA];
  const float* b_row[NBL];
  bool a_ok[NA], b_ok[NBL];
  const float *Ab = nullptr, *Bb = nullptr;
  int64_t lda = 0, ldb = 0;
  int Ks = 0, cur_src = -1;
  const float* safe = p.A[0];

  auto bind_src = [&](int src) __attribute__((always_inline)) {
    cur_src = src;
    Ks = (src == 0) ? kend0 : p.K[1];
    Ab = p.A[src] + zb * p.a_bs[src];
    Bb = p.B[src] + zb * p.b_bs[src];
    lda = p.lda[src]; ldb = p.ldb[src];
    if (!A_KM) {
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        const int gm = m0 + ((tid + 256 * i) >> 3);
        a_ok[i] = gm < Mlim;
        int64_t ridx = a_ok[i] ? gm : 0;
        if (a_ok[i] && p.a_idx[src]) ridx = p.a_idx[src][gm];
        a_row[i] = Ab + ridx * lda;
      }
    }
    if (!B_KM) {
#pragma unroll
      for (int i = 0; i < NBL; ++i) {
        const int f = tid + 256 * i;
        const int gn = n0 + (f >> 3);
        b_ok[i] = (f < TBN * 8) && gn < p.N;
        b_row[i] = Bb + (int64_t)(b_ok[i] ? gn : 0) * ldb;
      }
    }
  };
  auto load_tile = [&](int t, auto& a_reg, auto& b_reg) __attribute__((always_inline)) {
    const int src = t < T0 ? 0 : 1;
    if (src != cur_src) bind_src(src);
    const int k0 = (src == 0) ? kbeg + t * BK : (t - T0) * BK;
    if (!A_KM) {
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        const int k = k0 + 4 * ((tid + 256 * i) & 7);
        a_reg[i] = ld4<VEC>(a_row[i] + k, a_ok[i] ? Ks - k : 0, safe);
      }
    } else {
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        const int f = tid + 256 * i;
        const int k = k0 + (f / (TBM / 4));
        const int m = m0 + 4 * (f % (TBM / 4));
        a_reg[i] = ld4<VEC>(Ab + (int64_t)k * lda + m, k < Ks ? p.M - m : 0, safe);
      }
    }
    if (!B_KM) {
#pragma unroll
      for (int i = 0; i < NBL; ++i) {
        const int k = k0 + 4 * ((tid + 256 * i) & 7);
        b_reg[i] = ld4<VEC>(b_row[i] + k, b_ok[i] ? Ks - k : 0, safe);
      }
    } else {
#pragma unroll
      for (int i = 0; i < NBL; ++i) {
        const int f = tid + 256 * i;
        const int kr = f / NB4;
        const int k = k0 + kr;
        const int n = n0 + 4 * (f - kr * NB4);
        const bool ok = (f < BK * NB4) && k < Ks && n < p.N;
        int64_t krow = ok ? k : 0;
        if (ok && p.b_idx && src == 0) krow = p.b_idx[k];
        b_reg[i] = ld4<VEC>(Bb + krow * ldb + n, ok ? p.n_real - n : 0, safe);
        if (A_KM && ok && p.n_real < p.N) {
          // bias column: dW's extra column accumulates sum_k dY[k][m] * (scale[k] or 1)
          const int e = p.n_real - n;
          if (e >= 0 && e < 4) {
            const float one = 1.f;
            if (e == 0) b_reg[i].x = one; else if (e == 1) b_reg[i].y = one; else if (e == 2) b_reg[i].z = one; else b_reg[i].w = one;
          }
        }
      }
    }
  };
  auto store_tile = [&](int buf, const auto& a_reg, const auto& b_reg) __attribute__((always_inline)) {
    float* as = As[buf];
    float* bs = Bs[buf];
    if (!A_KM) {
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        const int f = tid + 256 * i;
        float* d = as + (f >> 3) * LDA_RM + 4 * (f & 7);
        *reinterpret_cast<float2*>(d) = float2{a_reg[i].x, a_reg[i].y};
        *reinterpret_cast<float2*>(d + 2) = float2{a_reg[i].z, a_reg[i].w};
      }
    } else {
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        const int f = tid + 256 * i;
        *reinterpret_cast<float4*>(as + (f / (TBM / 4)) * LDAK + 4 * (f % (TBM / 4))) = a_reg[i];
      }
    }
    if (!B_KM) {
#pragma unroll
      for (int i = 0; i < NBL; ++i) {
        const int f = tid + 256 * i;
        if (f < TBN * 8) {
          float* d = bs + (f >> 3) * LDA_RM + 4 * (f & 7);
          *reinterpret_cast<float2*>(d) = float2{b_reg[i].x, b_reg[i].y};
          *reinterpret_cast<float2*>(d + 2) = float2{b_reg[i].z, b_reg[i].w};
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < NBL; ++i) {
        const int f = tid + 256 * i;
        if (f < BK * NB4) {
          const int kr = f / NB4;
          *reinterpret_cast<float4*>(bs + kr * LDBK + 4 * (f - kr * NB4)) = b_reg[i];
        }
      }
    }
  };
  // fragments of k-step s (lane (r, g) holds A[row r][k = 4s + g], B[k = 4s + g][col r])
  auto load_frags = [&](const float* as, const float* bs, int s, float (&a)[NI], float (&b)[NJ]) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NI; ++i)
      a[i] = A_KM ? as[(4 * s + g) * LDAK + wrow + 16 * i + r] : as[(wrow + 16 * i + r) * LDA_RM + 4 * s + g];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int col = wcol + (SMALL ? 64 : 16) * j + r;
      b[j] = B_KM ? bs[(4 * s + g) * LDBK + col] : bs[col * LDA_RM + 4 * s + g];
    }
  };
  // a wavefront whose 16-row strip lies entirely beyond M issues no MFMAs for it (172-row weight-gradient tiles:
  // the matrix pipe of its SIMD is left to the co-resident workgroup)
  const bool strip_on[2] = {m0 + wrow < p.M, m0 + wrow + 16 < p.M};
  auto mma = [&](const float (&a)[NI], const float (&b)[NJ]) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NI; ++i)
      if (strip_on[i])
#pragma unroll
      for (int j = 0; j < NJ; ++j)
        if (!SMALL || wcol + 64 * j < TBN)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
  };
  // all 8 k-steps of a tile; LDS beyond K holds zeros, so the K tail needs no guard.  Fragment reads of step
  // s+1 are issued ahead of the MFMAs of step s.
  auto compute_tile = [&](int buf) __attribute__((always_inline)) {
    const float* as = As[buf];
    const float* bs = Bs[buf];
    float a0[NI], b0[NJ], a1[NI], b1[NJ];
    load_frags(as, bs, 0, a0, b0);
#pragma unroll
    for (int s = 0; s < BK / 4; s += 2) {
      load_frags(as, bs, s + 1, a1, b1);
      mma(a0, b0);
      if (s + 2 < BK / 4) load_frags(as, bs, s + 2, a0, b0);
      mma(a1, b1);
    }
  };

  if constexpr (TINY) {
    // The small problems (composite weights, their gradient chains) are a handful of workgroups beside the step's large
    // launches: a k-tile costs one memory round trip, not its 16 MFMAs per wavefront.  Two tiles of loads stay in flight
    // (two register sets; the loop is unrolled by two so that the sets are compile-time names).
    if (T > 0) {
      load_tile(0, a_reg, b_reg);
      if (T > 1) load_tile(1, a_reg2, b_reg2);
      store_tile(0, a_reg, b_reg);
      __syncthreads();
      for (int t = 0; t < T; t += 2) {
        if (t + 2 < T) load_tile(t + 2, a_reg, b_reg);
        compute_tile(0);
        __syncthreads();
        if (t + 1 < T) store_tile(0, a_reg2, b_reg2);
        __syncthreads();
        if (t + 1 < T) {
          if (t + 3 < T) load_tile(t + 3, a_reg2, b_reg2);
          compute_tile(0);
          __syncthreads();
          if (t + 2 < T) store_tile(0, a_reg, b_reg);
          __syncthreads();
        }
      }
    }
  } else if (T > 0) {
    load_tile(0, a_reg, b_reg);
    store_tile(0, a_reg, b_reg);
    __syncthreads();
    for (int t = 0; t < T; ++t) {
      const bool more = t + 1 < T;
      if (more) load_tile(t + 1, a_reg, b_reg);  // global loads in flight during the MFMAs below
      compute_tile(0);
      __syncthreads();        // every wavefront is done reading the tile
      if (more) store_tile(0, a_reg, b_reg);
      __syncthreads();
    }
  }

  // epilogue.  C/D layout of 16x16x4: col = lane & 15, row = 4*(lane >> 4) + reg
  float* Cb;
  int64_t ldc;
  const bool plain = (A_KM && p.nsplit > 1);
  if (plain) {
    Cb = p.slab_base + ((int64_t)zb * p.nsplit + split) * (int64_t)p.M * p.N;
    ldc = p.N;
  } else {
    Cb = p.C + zb * p.c_bs;
    ldc = p.ldc;
  }
  const float* bias = (p.bias && !plain) ? p.bias + zb * p.bias_bs : nullptr;
  const float* rs = (p.row_scale && !plain) ? p.row_scale + zb * p.rs_bs : nullptr;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int row = m0 + wrow + 16 * i + 4 * g + reg;
      if (row >= Mlim) continue;
      const float rscale = rs ? rs[(int64_t)row * p.rs_ld] : 1.f;
      const bool zero = (!plain && p.row_zero) ? (p.row_zero[row] != 0) : false;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int col = n0 + wcol + (SMALL ? 64 : 16) * j + r;
        if (col >= p.N || (SMALL && wcol + 64 * j >= TBN)) continue;
        float v = acc[i][j][reg];
        if (!plain) {
          if (p.accumulate) v += Cb[(int64_t)row * ldc + col];
          if (bias) v = fmaf(bias[col], rscale, v);
          if (zero) v = 0.f;
          if (p.relu) v = fmaxf(v, 0.f);
          if (p.relu_src) v = (p.relu_src[(int64_t)row * p.relu_ld + col] > 0.f) ? v : 0.f;
        }
        Cb[(int64_t)row * ldc + col] = v;
      }
    }
  }
}

#define GEMM_LDS_DECL                                                                    \
  __shared__ __attribute__((aligned(16))) float lds_a[AS_FLOATS]; \
  __shared__ __attribute__((aligned(16))) float lds_b[BS_FLOATS]

template <bool A_KM, bool B_KM, int TILE, bool VEC>
__global__ __launch_bounds__(GEMM_THREADS) void gemm_f32_kernel(const GemmDev p) {
  GEMM_LDS_DECL;
  int zb = blockIdx.z, split = 0;
  if (A_KM && p.nsplit > 1) { split = zb % p.nsplit; zb /= p.nsplit; }
  gemm_tile<A_KM, B_KM, TILE, VEC>(p, blockIdx.x, blockIdx.y, zb, split, lds_a, lds_b);
}

int gemm_f32_run(int form, bool vec, bool a_km, bool b_km, dim3 grid, dim3 block, const GemmDev& d, hipStream_t stream) {
#define GEMM_GO(A_KM, B_KM, TILE)                                                                                    \
  do {                                                                                                                \
    if (vec) PFO_KLAUNCH((gemm_f32_kernel<A_KM, B_KM, TILE, true>), grid, block, 0, stream, d);                      \
    else PFO_KLAUNCH((gemm_f32_kernel<A_KM, B_KM, TILE, false>), grid, block, 0, stream, d);                         \
  } while (0)
  switch (form) {
    case PFO_GEMM_FORM_F32_128:
      if (a_km) { if (b_km) GEMM_GO(true, true, 0); else GEMM_GO(true, false, 0); }
      else if (b_km) GEMM_GO(false, true, 0);
      else GEMM_GO(false, false, 0);
      break;
    case PFO_GEMM_FORM_F32_32: if (b_km) GEMM_GO(false, true, 1); else GEMM_GO(false, false, 1); break;
  }
#undef GEMM_GO
  PFO_LAUNCH_CHECK();
  return PFO_OK;
}

// ---------------------------------------------------------------------------------------------
// Several SMALL independent contractions in one launch (the composite-weight products of a layer and their
// gradient chain: each is far too small to fill the chip or to amortise a launch).  32 x 64 tiles; the operand
// layout is a per-problem switch (wavefront-uniform).
template <bool VEC>
__global__ __launch_bounds__(GEMM_THREADS) void gemm_multi_kernel(const MultiDev g) {
  // the 32 x 64 tile's staging: A max(32 * 34, 32 * 48), B max(64 * 34, 32 * 80) floats - 16 KB, so these launches take
  // little room beside the large ones they run next to
  __shared__ __attribute__((aligned(16))) float lds_a[1536];
  __shared__ __attribute__((aligned(16))) float lds_b[2560];
  int q = 0;
#pragma unroll
  for (int i = 1; i < MULTI_MAX; ++i)
    if (i < g.n && (int)blockIdx.x >= g.tile_begin[i]) q = i;
  int t = blockIdx.x - g.tile_begin[q];
  const int per_batch = g.tm[q] * g.tn[q];
  const int zb = t / per_batch;
  t -= zb * per_batch;
  const int bx = t / g.tn[q], by = t % g.tn[q];
  const GemmDev p = g.p[q];                       // a copy: indexing the by-value argument through a reference costs scratch
  switch (g.layout[q]) {
    case 0: gemm_tile<false, false, 2, VEC>(p, bx, by, zb, 0, lds_a, lds_b); break;
    case 1: gemm_tile<false, true, 2, VEC>(p, bx, by, zb, 0, lds_a, lds_b); break;
    case 2: gemm_tile<true, false, 2, VEC>(p, bx, by, zb, 0, lds_a, lds_b); break;
    default: gemm_tile<true, true, 2, VEC>(p, bx, by, zb, 0, lds_a, lds_b); break;
  }
}

int gemm_multi_run(bool vec, dim3 grid, const MultiDev& g, hipStream_t stream) {
  if (vec) PFO_KLAUNCH(gemm_multi_kernel<true>, grid, dim3(GEMM_THREADS), 0, stream, g);
  else PFO_KLAUNCH(gemm_multi_kernel<false>, grid, dim3(GEMM_THREADS), 0, stream, g);
  PFO_LAUNCH_CHECK();
  return PFO_OK;
}

// ---------------------------------------------------------------------------------------------
// The grouped weight gradients (gemm_dev.hpp TnGroupDev) on this tile
// (scalar loads: operands that admit float4 loads take gemm_tn_group_bx_kernel, gemm_tn_bx.hip)
__global__ __launch_bounds__(GEMM_THREADS) void gemm_tn_group_kernel(const TnGroupDev g) {
  GEMM_LDS_DECL;
  int q = 0;
#pragma unroll
  for (int i = 1; i < TN_MAX_PROBLEMS; ++i)
    if (i < g.n && (int)blockIdx.x >= g.p[i].tile_begin) q = i;
  const TnProbDev& pr = g.p[q];
  const int t = blockIdx.x - pr.tile_begin;
  GemmDev d;
  d.A[0] = pr.A; d.A[1] = nullptr; d.lda[0] = pr.lda; d.lda[1] = 0; d.a_idx[0] = d.a_idx[1] = nullptr;
  d.B[0] = pr.B; d.B[1] = nullptr; d.ldb[0] = pr.ldb; d.ldb[1] = 0; d.b_idx = pr.b_idx;
  d.K[0] = g.K; d.K[1] = 0;
  d.C = nullptr; d.ldc = 0; d.bias = nullptr; d.row_scale = nullptr; d.rs_ld = 0; d.row_zero = nullptr;
  d.relu_src = nullptr; d.relu_ld = 0; d.M = pr.M; d.N = pr.N; d.m_dev = g.k_dev; d.relu = 0; d.accumulate = 0;
  d.add_src = nullptr; d.add_ld = 0; d.add_idx = nullptr;
  d.nsplit = g.nsplit > 1 ? g.nsplit : 2;   // any value > 1 selects the slab epilogue; the split index comes from blockIdx.y
  d.split_chunk = g.chunk;
  d.a_bs[0] = d.a_bs[1] = d.b_bs[0] = d.b_bs[1] = d.c_bs = d.bias_bs = d.rs_bs = 0;
  d.n_real = pr.N_real;
  // slab region of this problem: [nsplit][M][N]; gemm_tile indexes it as (zb * nsplit + split) with zb = 0
  d.slab_base = g.slabs + pr.slab_off;
  d.dyn_chunk = (g.k_dev != nullptr && g.nsplit > 1) ? 1 : 0;
  gemm_tile<true, true, 0, false>(d, t / pr.tn, t % pr.tn, 0, blockIdx.y, lds_a, lds_b);
}
int gemm_tn_group_f32_run(dim3 grid, dim3 block, const TnGroupDev& g, hipStream_t stream) {
  PFO_KLAUNCH(gemm_tn_group_kernel, grid, block, 0, stream, g);
  PFO_LAUNCH_CHECK();
  return PFO_OK;
}

// ---------------------------------------------------------------------------------------------
// out[m, n] += sum_r u_r[m] * v_r[n], several independent updates in one launch (blockIdx.y = the update)
struct Rank1Dev {
  const float* u[PFO_RANK1_MAX]; const float* v[PFO_RANK1_MAX]; float* out[PFO_RANK1_MAX];
  int64_t ldu[PFO_RANK1_MAX], ldv[PFO_RANK1_MAX], ldo[PFO_RANK1_MAX], u_rs[PFO_RANK1_MAX], v_rs[PFO_RANK1_MAX];
  int M[PFO_RANK1_MAX], N[PFO_RANK1_MAX], reps[PFO_RANK1_MAX];
};
__global__ void rank1_kernel(const Rank1Dev g) {
  const int q = blockIdx.y;
  const int N = g.N[q], reps = g.reps[q];
  const int64_t total = (int64_t)g.M[q] * N;
  const float* __restrict__ u = g.u[q];
  const float* __restrict__ v = g.v[q];
  float* __restrict__ out = g.out[q];
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int m = (int)(e / N), n = (int)(e - (int64_t)m * N);
    float acc = 0.f;
    for (int r = 0; r < reps; ++r) acc = fmaf(u[r * g.u_rs[q] + (int64_t)m * g.ldu[q]], v[r * g.v_rs[q] + (int64_t)n * g.ldv[q]], acc);
    out[(int64_t)m * g.ldo[q] + n] += acc;
  }
}
int pfo_rank1_multi_launch(const PfoRank1* list, int n, hipStream_t stream) {
  PFO_REQUIRE(list && n >= 1 && n <= PFO_RANK1_MAX, "bad rank-1 list");
  Rank1Dev g;
  int64_t most = 0;
  for (int i = 0; i < n; ++i) {
    const PfoRank1& r = list[i];
    PFO_REQUIRE(r.u && r.v && r.out && r.M > 0 && r.N > 0 && r.reps >= 1, "bad rank-1 update");
    g.u[i] = r.u; g.v[i] = r.v; g.out[i] = r.out; g.ldu[i] = r.ldu; g.ldv[i] = r.ldv; g.ldo[i] = r.ldo; g.M[i] = r.M; g.N[i] = r.N;
    g.reps[i] = r.reps; g.u_rs[i] = r.u_rs; g.v_rs[i] = r.v_rs;
    most = std::max(most, (int64_t)r.M * r.N);
  }
  const int nb = (int)std::min<int64_t>(512, pfo_ceil_div(most, 256));
  PFO_KLAUNCH(rank1_kernel, dim3(nb, n), dim3(256), 0, stream, g);
  PFO_LAUNCH_CHECK();
  return PFO_OK;
}
// dst[i] (+)= sum_s src[s * stride + i]  (fixed order: reproducible), several destinations in one launch
struct SumSlabsDev {
  float* dst[PFO_SUM_SLABS_MAX]; const float* src[PFO_SUM_SLABS_MAX];
  int64_t stride[PFO_SUM_SLABS_MAX], count[PFO_SUM_SLABS_MAX];
  int n_slabs[PFO_SUM_SLABS_MAX], accumulate[PFO_SUM_SLABS_MAX];
};
__global__ void sum_slabs_kernel(const SumSlabsDev g) {
  const int q = blockIdx.y;
  const float* __restrict__ src = g.src[q];
  float* __restrict__ dst = g.dst[q];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < g.count[q]; i += (int64_t)gridDim.x * blockDim.x) {
    float acc = g.accumulate[q] ? dst[i] : 0.f;
    for (int sl = 0; sl < g.n_slabs[q]; ++sl) acc += src[sl * g.stride[q] + i];
    dst[i] = acc;
  }
}
int pfo_sum_slabs_launch(const PfoSumSlabs* list, int n, hipStream_t stream) {
  PFO_REQUIRE(list && n >= 1 && n <= PFO_SUM_SLABS_MAX, "bad slab list");
  SumSlabsDev g;
  int64_t most = 0;
  for (int i = 0; i < n; ++i) {
    PFO_REQUIRE(list[i].dst && list[i].src && list[i].count > 0 && list[i].n_slabs >= 1, "bad slab sum");
    g.dst[i] = list[i].dst; g.src[i] = list[i].src; g.stride[i] = list[i].stride; g.count[i] = list[i].count;
    g.n_slabs[i] = list[i].n_slabs; g.accumulate[i] = list[i].accumulate;
    most = std::max(most, list[i].count);
  }
  const int nb = (int)std::min<int64_t>(256, pfo_ceil_div(most, 256));
  PFO_KLAUNCH(sum_slabs_kernel, dim3(nb, n), dim3(256), 0, stream, g);
  PFO_LAUNCH_CHECK();
  return PFO_OK;
}
int pfo_rank1_launch(const float* u, int64_t ldu, const float* v, int64_t ldv, int M, int N, float* out, int64_t ldo,
                     hipStream_t stream) {
  PfoRank1 r;
  r.u = u; r.ldu = ldu; r.v = v; r.ldv = ldv; r.M = M; r.N = N; r.out = out; r.ldo = ldo;
  return pfo_rank1_multi_launch(&r, 1, stream);
}
