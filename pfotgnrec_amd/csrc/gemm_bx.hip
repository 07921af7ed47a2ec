// The image kernels: C = A op(B) for a row-major fp32 A against the pre-split image of B (bimg.hip) on the fp16 matrix cores,
// two fp16 pieces per element and three products per block (gemm_dev.hpp).  Three 128-row forms (areg, areg8, astat) and the
// 32-row one for short operands; gemm.hip's plan names the form, gemm_bx_run at the end launches it.
#include "gemm_dev.hpp"

#define BX_B_PIECE (BN * 64)       // bytes of one piece of a B image tile
#define BX_AREG_OCC 2
#define SK_A_PIECE (SK_ROWS * 64)

// ---------------------------------------------------------------------------------------------
// The 128-row form: the A tile never touches LDS.  Every wavefront loads the 32 rows it owns
// straight in MFMA fragment order (lane (r, g): row r, k = 8g..8g+7 = two float4), splits them in registers into the
// two fp16 fragments, and only the shared B image goes through LDS - double-buffered, so a k-tile costs ONE barrier
// and the copy of tile t+1 into the other buffer runs beside the MFMAs of tile t.
template <int WAVES, int FMT, int S = 2>
__device__ __forceinline__ void bx_areg_body(const GemmDev& p, char* lds) {
  constexpr int NP = BxFmt<FMT>::NP;
  constexpr int NTHR = 64 * WAVES;                   // threads per workgroup; S strips of 16 rows per wavefront
  constexpr int UNITS = NP * (BX_B_PIECE / 16);      // 16-byte units of one B image tile (a multiple of 64)
  constexpr int NDMA = (UNITS + NTHR - 1) / NTHR;    // rounds of 16-byte units per thread
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  int tile_m = blockIdx.x, tile_n = blockIdx.y;
  if (p.xcd_tn > 0 && !xcd_tile(blockIdx.x, p.xcd_tm, p.xcd_tn, tile_m, tile_n)) return;
  const int m0 = tile_m * (16 * S * WAVES), n0 = tile_n * BN;
  int Mlim = p.M;
  if (p.m_dev) Mlim = min(Mlim, *p.m_dev);
  if (m0 >= Mlim || n0 >= p.N) return;
  const int wrow = 16 * S * wave;

  f32x4 acc[S][11];
#pragma unroll
  for (int i = 0; i < S; ++i)
#pragma unroll
    for (int j = 0; j < 11; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int T0 = (p.K[0] + BK - 1) / BK;
  const int T1 = (p.K[1] > 0 && p.A[1]) ? (p.K[1] + BK - 1) / BK : 0;
  const int T = T0 + T1;
  const float* safe = p.A[0];
  const int64_t img_piece = (int64_t)p.b_img_rows * 64;
  // rows of this lane (one per strip) for both sources
  const float* a_row[2][S];
  bool a_ok[S];
#pragma unroll
  for (int i = 0; i < S; ++i) {
    const int gm = m0 + wrow + 16 * i + r;
    a_ok[i] = gm < Mlim;
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      int64_t ridx = a_ok[i] ? gm : 0;
      if (a_ok[i] && (s2 == 0 || T1 > 0) && p.a_idx[s2]) ridx = p.a_idx[s2][gm];
      a_row[s2][i] = (s2 == 0 || T1 > 0) ? p.A[s2] + ridx * p.lda[s2] + 8 * g : p.A[0];
    }
  }
  const char* img[2] = {reinterpret_cast<const char*>(p.b_img) + (int64_t)n0 * 64,
                        T1 > 0 ? reinterpret_cast<const char*>(p.b_img2) + (int64_t)n0 * 64 : nullptr};
  // FMT 1: exponents of the image rows (this block's columns) behind the tiles of each image
  const int32_t* bexp[2] = {reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(p.b_img) + (int64_t)T0 * NP * img_piece) + n0,
                            T1 > 0 ? reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(p.b_img2) + (int64_t)T1 * NP * img_piece) + n0
                                   : nullptr};

  float4 a_raw[2][S][2];              // [set][strip][half]: k = k0 + 8g + 4*half ..; tile t lives in set t & 1
  typedef __attribute__((address_space(1))) const void* gptr_t;
  typedef __attribute__((address_space(3))) void* lptr_t;
  // A rows of tile t -> registers, two tiles ahead of the MFMAs (HBM latency under load exceeds one k-tile of MFMAs now that a
  // tile is 66 of them)
  auto load_a = [&](int t, auto setc) {
    constexpr int set = decltype(setc)::value;
    const int src = t < T0 ? 0 : 1;
    const int ts = src == 0 ? t : t - T0;
    const int k = ts * BK + 8 * g;
    const int Ks = p.K[src];
    const int toff = ts * BK;
#pragma unroll
    for (int i = 0; i < S; ++i)
#pragma unroll
      for (int h = 0; h < 2; ++h)
        a_raw[set][i][h] = ld4<true>(a_row[src][i] + toff + 4 * h, a_ok[i] ? Ks - (k + 4 * h) : 0, safe);
  };
  // B image tile -> LDS by asynchronous global->LDS loads (the LDS image IS the global image: a lane-linear copy, no
  // staging registers, no ds_write); `buf` is the buffer being filled for tile t
  auto load_b = [&](int t, int buf) {
    const int src = t < T0 ? 0 : 1;
    const int ts = src == 0 ? t : t - T0;
    const char* tile = img[src] + (int64_t)ts * NP * img_piece;
    char* Bs = lds + buf * NP * BX_B_PIECE;
    bx_for<NDMA>([&](auto uc) {
      constexpr int u = decltype(uc)::value;
      const int unit0 = 64 * wave + NTHR * u;                  // the last round covers some of the wavefronts only (wave-uniform)
      if (unit0 < UNITS) {
        const int unit = unit0 + lane;
        const int q = unit / (BX_B_PIECE / 16);
        __builtin_amdgcn_global_load_lds((gptr_t)(tile + q * img_piece + (unit - q * (BX_B_PIECE / 16)) * 16),
                                         (lptr_t)(Bs + unit0 * 16), 16, 0, 0);
      }
    });
  };
  u32x4 a[S][NP];
  int rowE[S];
#pragma unroll
  for (int i = 0; i < S; ++i) rowE[i] = HX_EMIN;    // FMT 1: biased exponent of the running maximum of this lane's two rows
  auto split_a = [&](auto setc, bool first) {
    bx_split_rows<FMT, 11, S>(a_raw[decltype(setc)::value], a, rowE, acc, first);
  };
  const int frag_off = r * 64 + ((g ^ bx_swz(r)) << 4);
  auto compute_tile = [&](int buf) {
    const char* Bs = lds + buf * NP * BX_B_PIECE;
    auto ldb = [&](u32x4 (&b)[NP], int j) {
#pragma unroll
      for (int q = 0; q < NP; ++q) b[q] = *reinterpret_cast<const u32x4*>(Bs + q * BX_B_PIECE + (16 * j) * 64 + frag_off);
    };
    auto mma = [&](const u32x4 (&b)[NP], int j) {
#pragma unroll
      for (int i = 0; i < S; ++i) acc[i][j] = bx_mma<FMT>(b, a[i], acc[i][j]);     // operands swapped: image rows = accumulator columns
    };
    if constexpr (S == 1) {
      // one strip: the products of a column tile are ONE dependent chain - two column tiles are multiplied product by product
      // in turn, and the fragments of the next pair are read meanwhile (four register sets)
      constexpr int NQ = 3;
      u32x4 bb[4][NP];
      ldb(bb[0], 0); ldb(bb[1], 1);
      bx_for<6>([&](auto pc) {
        constexpr int j = 2 * decltype(pc)::value, cs = (decltype(pc)::value & 1) * 2;
        if constexpr (j + 2 < 11) ldb(bb[2 - cs], j + 2);
        if constexpr (j + 3 < 11) ldb(bb[3 - cs], j + 3);
        bx_for<NQ>([&](auto qc) {
          constexpr int Q = decltype(qc)::value;
          acc[0][j] = bx_mma_q<FMT, Q>(bb[cs], a[0], acc[0][j]);
          if constexpr (j + 1 < 11) acc[0][j + 1] = bx_mma_q<FMT, Q>(bb[cs + 1], a[0], acc[0][j + 1]);
        });
      });
    } else {
    u32x4 b0[NP], b1[NP];
    ldb(b0, 0);
#pragma unroll
    for (int j = 0; j < 11; j += 2) {
      if (j + 1 < 11) ldb(b1, j + 1);
      mma(b0, j);
      if (j + 2 < 11) ldb(b0, j + 2);
      if (j + 1 < 11) mma(b1, j + 1);
    }
    }
  };

  using C0 = std::integral_constant<int, 0>;
  using C1 = std::integral_constant<int, 1>;
  // one k-tile: the fragments of tile t are in `a`; queue the image of t+1 and the rows of t+2, multiply, split the rows of t+1
  auto step = [&](int t, auto curc) {
    constexpr int cur = decltype(curc)::value;                 // == t & 1
    const bool more = t + 1 < T, more2 = t + 2 < T;
    if (more) load_b(t + 1, (t + 1) & 1);
    if (more2) load_a(t + 2, curc);                            // (the raw rows of tile t were split before this call)
    if constexpr (FMT == 1) {
      if (t == T0 && T1 > 0) {                     // second source: its image rows have their own scales - move the sums over
#pragma unroll
        for (int j = 0; j < 11; ++j) {
          const int4 e1 = *reinterpret_cast<const int4*>(bexp[0] + 16 * j + 4 * g);
          const int4 e2 = *reinterpret_cast<const int4*>(bexp[1] + 16 * j + 4 * g);
          const int4 d = {e1.x - e2.x, e1.y - e2.y, e1.z - e2.z, e1.w - e2.w};
#pragma unroll
          for (int i = 0; i < S; ++i) acc[i][j] = hx_scale4(acc[i][j], d, 0);
        }
      }
    }
    compute_tile(cur);
    if (more) {
      // the DMA is ordered only by the issuing wave's vmcnt + the barrier; the four row loads of tile t+2 were issued last
      if (more2) { if constexpr (S == 2) asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); }
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      split_a(std::integral_constant<int, 1 - cur>{}, false);  // this wavefront's own fragments for tile t+1
    }
    __syncthreads();
  };
  if (T > 0) {
    load_a(0, C0{});
    load_b(0, 0);
    if (T > 1) { load_a(1, C1{}); if constexpr (S == 2) asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); }
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    split_a(C0{}, true);
    __syncthreads();
    for (int t = 0; t < T; t += 2) {
      step(t, C0{});
      if (t + 1 < T) step(t + 1, C1{});
    }
  }

  float* Cb = p.C;
  const int64_t ldc = p.ldc;
  const float* bias = p.bias;
  const float* rs = p.row_scale;
  const bool n4 = bx_n4(p, Cb, ldc, bias);
  const int32_t* bexp_last = T1 > 0 ? bexp[1] : bexp[0];
  if (n4) {
    // Every load of the epilogue BEFORE the first store.  The compiler may not move a load above a store that could alias it,
    // so "load the column's exponents, scale, store" 22 times over was a chain of 22 load latencies per wavefront, each behind
    // the previous store (in-kernel stamps, profiles/r5_areg_stamps.txt: 11 of a workgroup's 25 us at the d ctx' shape).
    // Per-COLUMN values (image-row exponents, bias) go through LDS - the image buffers are free after the last k-tile's
    // barrier; per-ROW sources (accumulate / addend rows / ReLU source) are read one source at a time for both strips.
    int* s_exp = reinterpret_cast<int*>(lds);
    float* s_bias = reinterpret_cast<float*>(lds) + BN;
    for (int c = tid; c < BN; c += NTHR) {
      const bool in = n0 + c < p.N;
      if constexpr (FMT == 1) s_exp[c] = in ? bexp_last[c] : 0;
      s_bias[c] = (bias && in) ? bias[n0 + c] : 0.f;
    }
    __syncthreads();
    int row[S]; bool ok[S];
#pragma unroll
    for (int i = 0; i < S; ++i) { row[i] = m0 + wrow + 16 * i + r; ok[i] = row[i] < Mlim; if (!ok[i]) row[i] = m0; }
    float rscale[S];
#pragma unroll
    for (int i = 0; i < S; ++i) rscale[i] = rs ? rs[(int64_t)row[i] * p.rs_ld] : 1.f;
#pragma unroll
    for (int i = 0; i < S; ++i)
#pragma unroll
      for (int j = 0; j < 11; ++j) {
        const int c = 16 * j + 4 * g;
        if constexpr (FMT == 1) acc[i][j] = hx_scale4(acc[i][j], *reinterpret_cast<const int4*>(s_exp + c), rowE[i] - 2 * HX_TOP);
      }
    auto each_row_source = [&](const float* src, int64_t ld, const int32_t* idx, auto&& apply) {
      const float* rp[S];
#pragma unroll
      for (int i = 0; i < S; ++i) rp[i] = src + (int64_t)(idx ? idx[row[i]] : row[i]) * ld + n0 + 4 * g;
      const int lastc = p.N - n0 - 4 - 4 * g;                  // offset of the last in-range float4 from rp (n4: N is a multiple of 4)
      float4 t[S][11];                                         // (columns past N: the row's last four instead - never stored)
#pragma unroll
      for (int i = 0; i < S; ++i)
#pragma unroll
        for (int j = 0; j < 11; ++j) t[i][j] = *reinterpret_cast<const float4*>(rp[i] + min(16 * j, lastc));
#pragma unroll
      for (int i = 0; i < S; ++i)
#pragma unroll
        for (int j = 0; j < 11; ++j) apply(acc[i][j], t[i][j]);
    };
    if (p.accumulate) each_row_source(Cb, ldc, nullptr, [](f32x4& a, const float4 o) { a[0] += o.x; a[1] += o.y; a[2] += o.z; a[3] += o.w; });
    if (bias) {
#pragma unroll
      for (int i = 0; i < S; ++i)
#pragma unroll
        for (int j = 0; j < 11; ++j) {
          const float4 bv = *reinterpret_cast<const float4*>(s_bias + 16 * j + 4 * g);
          acc[i][j][0] = fmaf(bv.x, rscale[i], acc[i][j][0]); acc[i][j][1] = fmaf(bv.y, rscale[i], acc[i][j][1]);
          acc[i][j][2] = fmaf(bv.z, rscale[i], acc[i][j][2]); acc[i][j][3] = fmaf(bv.w, rscale[i], acc[i][j][3]);
        }
    }
    if (p.add_src) each_row_source(p.add_src, p.add_ld, p.add_idx, [](f32x4& a, const float4 o) { a[0] += o.x; a[1] += o.y; a[2] += o.z; a[3] += o.w; });
    if (p.row_zero) {
#pragma unroll
      for (int i = 0; i < S; ++i)
        if (p.row_zero[row[i]] != 0) {
#pragma unroll
          for (int j = 0; j < 11; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    if (p.relu) {
#pragma unroll
      for (int i = 0; i < S; ++i)
#pragma unroll
        for (int j = 0; j < 11; ++j)
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[i][j][c] = fmaxf(acc[i][j][c], 0.f);
    }
    if (p.relu_src) each_row_source(p.relu_src, p.relu_ld, nullptr, [](f32x4& a, const float4 m) {
      a[0] = m.x > 0.f ? a[0] : 0.f; a[1] = m.y > 0.f ? a[1] : 0.f; a[2] = m.z > 0.f ? a[2] : 0.f; a[3] = m.w > 0.f ? a[3] : 0.f; });
#pragma unroll
    for (int i = 0; i < S; ++i) {
      if (!ok[i]) continue;
      float* cp = Cb + (int64_t)row[i] * ldc + n0 + 4 * g;
#pragma unroll
      for (int j = 0; j < 11; ++j)
        if (n0 + 16 * j + 4 * g < p.N) *reinterpret_cast<f32x4*>(cp + 16 * j) = acc[i][j];
    }
  } else {
#pragma unroll
  for (int i = 0; i < S; ++i) {
    const int row = m0 + wrow + 16 * i + r;
    if (row >= Mlim) continue;
    const float rscale = rs ? rs[(int64_t)row * p.rs_ld] : 1.f;
    const bool zero = p.row_zero ? (p.row_zero[row] != 0) : false;
    const float* addrow = p.add_src ? p.add_src + (int64_t)(p.add_idx ? p.add_idx[row] : row) * p.add_ld : nullptr;
#pragma unroll
    for (int j = 0; j < 11; ++j) {
      const int col = n0 + 16 * j + 4 * g;
      if (col < p.N) {
        f32x4 v = acc[i][j];
        if constexpr (FMT == 1) v = hx_scale4(v, *reinterpret_cast<const int4*>(bexp_last + 16 * j + 4 * g), rowE[i] - 2 * HX_TOP);
        bx_store4(p, Cb, ldc, bias, rscale, zero, n4, row, col, v, addrow);
      }
    }
  }
  }
}
template <int FMT>
__global__ __launch_bounds__(GEMM_THREADS, FMT == 1 ? BX_AREG_OCC : 2) void gemm_bx_areg_kernel(const GemmDev p) {
  __shared__ __attribute__((aligned(16))) char lds[2 * BxFmt<FMT>::NP * BX_B_PIECE];
  bx_areg_body<4, FMT>(p, lds);
}
// The same 128-row workgroup as EIGHT wavefronts of one 16-row strip each: half the registers per wavefront (<= 128), so four
// wavefronts per SIMD instead of two - the row split (vector pipe) of one wavefront runs beside the MFMAs of another and a
// wavefront waiting for its rows leaves three to issue.  In-kernel stamps of the four-wavefront form (profiles/r5_areg_stamps.txt):
// per k-tile 1 370 cycles of MFMAs, 330 waiting for rows, 650-740 splitting rows, 150-180 at the barrier, one after the other.
template <int FMT>
__global__ __launch_bounds__(512, 2) void gemm_bx_areg8_kernel(const GemmDev p) {
  __shared__ __attribute__((aligned(16))) char lds[2 * BxFmt<FMT>::NP * BX_B_PIECE];
  bx_areg_body<8, FMT, 1>(p, lds);
}
// ---------------------------------------------------------------------------------------------
// A-STATIONARY form of the image kernel for SHORT contractions with MANY output columns (the d ctx' contraction: K = 172,
// N = 704): a wavefront loads its 32 rows ONCE, finds each row's scale from the whole row (no running maximum, no rescaling),
// splits them into the fp16 fragments of ALL k-tiles (<= 6 tiles: 96 registers) and keeps them; the image of B then streams
// through an LDS ring, two 16-column tiles per slot, and every pair of column tiles is multiplied, scaled and STORED while the
// next ones arrive.  Against gemm_bx_areg_kernel on this shape (in-kernel stamps, profiles/r5_areg_stamps.txt): the rows are
// read and split once instead of once per 176-column block (4 x), the 3 us of load latency in front of a workgroup's first MFMA
// is paid once per 128 x 704 instead of per 128 x 176 output, and the stores leave evenly over the workgroup's life instead of
// in a burst behind its last k-tile (workgroups of one launch run in lockstep: everyone stored at once, nobody multiplied).
// Plain stores only (no bias / addend / ReLU epilogue), N a multiple of 32, K <= 192, fp16x2 format; a workgroup whose 128 rows
// are not all inside M takes conservative waits (the exact vmcnt bookkeeping below assumes no store is skipped).
#define AS_RING 3
template <bool FULL, int T>
__device__ __forceinline__ void bx_astat_body(const GemmDev& p, char* lds) {
  constexpr int NP = 2;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int m0 = blockIdx.x * 128;
  int Mlim = p.M;
  if (p.m_dev) Mlim = min(Mlim, *p.m_dev);
  const int wrow = 32 * wave;
  const int K = p.K[0];
  const int NS = p.N >> 5;                                         // slots: pairs of column tiles
  const int64_t img_piece = (int64_t)p.b_img_rows * 64;
  const char* img = reinterpret_cast<const char*>(p.b_img);
  const int slot_bytes = 4 * T * 1024;                             // [column tile 0 | 1][k-tile][piece] x (16 image rows x 64 B)
  char* ring = lds;
  const int32_t* bexp = reinterpret_cast<const int32_t*>(img + (int64_t)T * NP * img_piece);   // the image rows' exponents
  typedef __attribute__((address_space(1))) const void* gptr_t;
  typedef __attribute__((address_space(3))) void* lptr_t;
  // chunk c of a slot = (column tile jj, k-tile t, piece q), c = (jj * T + t) * 2 + q: 1 KB, contiguous in the image; wavefront w
  // moves the chunks w, w + 4, ... (T of them)
  auto dma_slot = [&](int s) {
    char* dst = ring + (s % AS_RING) * (4 * AS_TMAX * 1024);
    bx_for<T>([&](auto uc) {                                        // exactly T instructions per wavefront (the vmcnt bookkeeping counts them)
      const int c = wave + 4 * decltype(uc)::value;
      const int q = c & 1, h = c >> 1, jj = h >= T ? 1 : 0, t = h - jj * T;
      const char* src = img + ((int64_t)t * NP + q) * img_piece + (int64_t)(32 * s + 16 * jj) * 64;
      __builtin_amdgcn_global_load_lds((gptr_t)(src + lane * 16), (lptr_t)(dst + c * 1024), 16, 0, 0);
    });
  };
  // ---- the rows: loaded once, scaled by the row's own maximum, split for every k-tile
  u32x4 a[AS_TMAX][2][NP];
  int rowE[2];
  {
    float4 raw[AS_TMAX][2][2];
    const float* a_row[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int gm = m0 + wrow + 16 * i + r;
      int64_t ridx = (FULL || gm < Mlim) ? gm : m0;
      if (p.a_idx[0]) ridx = p.a_idx[0][ridx];
      a_row[i] = p.A[0] + ridx * p.lda[0] + 8 * g;
    }
#pragma unroll
    for (int t = 0; t < AS_TMAX; ++t)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int k = t * BK + 8 * g + 4 * h;
          raw[t][i][h] = (t < T && k < K) ? *reinterpret_cast<const float4*>(a_row[i] + t * BK + 4 * h) : float4{0.f, 0.f, 0.f, 0.f};
        }
    // (behind the row loads in program order: the first MFMA needs both, and the rows come from HBM)
    dma_slot(0);
    if (NS > 1) dma_slot(1);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      float mx = 0.f;
#pragma unroll
      for (int t = 0; t < AS_TMAX; ++t) mx = fmaxf(mx, hx_absmax8(raw[t][i][0], raw[t][i][1]));
      rowE[i] = hx_exp_of_bits(hx_max_over_g(__float_as_uint(mx)));
      const int se = HX_TOP - rowE[i];
#pragma unroll
      for (int t = 0; t < AS_TMAX; ++t) {
        uint2 h0, l0, h1, l1;
        hx_split4(raw[t][i][0], se, h0, l0);
        hx_split4(raw[t][i][1], se, h1, l1);
        a[t][i][0] = u32x4{h0.x, h0.y, h1.x, h1.y};
        a[t][i][1] = u32x4{l0.x, l0.y, l1.x, l1.y};
      }
    }
  }
  const int frag_off = r * 64 + ((g ^ bx_swz(r)) << 4);
  float* crow[2];
  bool ok[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = m0 + wrow + 16 * i + r;
    ok[i] = FULL || row < Mlim;
    crow[i] = p.C + (int64_t)(ok[i] ? row : m0) * p.ldc + 4 * g;
  }
  f32x4 prev[2][2];                                                // the pair of column tiles multiplied one slot ago, stored in this one
  int4 pexp[2];                                                    // ... and its columns' exponents, fetched one slot ahead (2 loads)
  // vmcnt bookkeeping of one wavefront, oldest first, at the top of slot s:
  //   ... DMA(s) [T] | stores(s-2) [4] | exponents(s-1) [2] | DMA(s+1) [T]
  // (iteration s-2 ended with DMA(s); iteration s-1 issued stores(s-2), the exponent loads of slot s-1, DMA(s+1)): DMA(s) has
  // landed when at most 4 + 2 + T younger operations are outstanding.  Members that do not exist (no stores before slot 2, no
  // DMA behind the last slot) are not counted: counting something that was never issued would make the wait too lax.
  auto wait_vm = [&](auto nc) {
    constexpr int n = FULL ? decltype(nc)::value : 0;
    static_assert(n <= 12, "vmcnt");
    if constexpr (n == 12) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
    else if constexpr (n == 11) asm volatile("s_waitcnt vmcnt(11)" ::: "memory");
    else if constexpr (n == 10) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
    else if constexpr (n == 9) asm volatile("s_waitcnt vmcnt(9)" ::: "memory");
    else if constexpr (n == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if constexpr (n == 7) asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
    else if constexpr (n == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else if constexpr (n == 5) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
    else if constexpr (n == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else if constexpr (n == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
    else if constexpr (n == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else if constexpr (n == 1) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  };
  // One slot: wait, barrier, then ONE straight-line block in which the 12 memory instructions of the slot (4 stores of the pair
  // multiplied one slot ago, 2 exponent loads, T DMA chunks of slot s+2) are spread between the k-tiles' MFMAs.  Issued in a
  // burst behind the barrier - by all four wavefronts at once - they queued in the CU's one texture-address unit for 1 430
  // cycles per slot while no wavefront multiplied (in-kernel stamps, profiles/r5_areg_stamps.txt).
  auto slot_body = [&](int s, auto hsc, auto hdc, auto nc) {
    constexpr bool HS = decltype(hsc)::value, HD = decltype(hdc)::value;
    wait_vm(nc);
    __syncthreads();                                               // DMA(s) of every wavefront has landed; slot (s-1) % RING is free
    const char* Bs = ring + (s % AS_RING) * (4 * AS_TMAX * 1024);
    char* dst = ring + ((s + 2) % AS_RING) * (4 * AS_TMAX * 1024);
    f32x4 acc[2][2];
#pragma unroll
    for (int jj = 0; jj < 2; ++jj)
#pragma unroll
      for (int i = 0; i < 2; ++i) acc[jj][i] = f32x4{0.f, 0.f, 0.f, 0.f};
    u32x4 b0[2][NP], b1[2][NP];
    auto ldb = [&](u32x4 (&b)[2][NP], int t) {
#pragma unroll
      for (int jj = 0; jj < 2; ++jj)
#pragma unroll
        for (int q = 0; q < NP; ++q) b[jj][q] = *reinterpret_cast<const u32x4*>(Bs + ((jj * T + t) * 2 + q) * 1024 + frag_off);
    };
    auto mma = [&](const u32x4 (&b)[2][NP], auto tc) {
      constexpr int t = decltype(tc)::value;
      // four independent accumulators, product by product: a dependent MFMA never follows its predecessor directly
      bx_for<3>([&](auto qc) {
        constexpr int Q = decltype(qc)::value;
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
#pragma unroll
          for (int i = 0; i < 2; ++i) acc[jj][i] = bx_mma_q<1, Q>(b[jj], a[t][i], acc[jj][i]);
      });
    };
    // memory instruction m of the slot, in the order the bookkeeping above assumes: 0..3 stores (jj, i) | 4, 5 exponents | 6.. DMA
    int4 nexp[2];
    auto mem_op = [&](auto mc) {
      constexpr int m = decltype(mc)::value;
      if constexpr (m < 4) {
        if constexpr (HS) {
          constexpr int jj = m >> 1, i = m & 1;
          const f32x4 v = hx_scale4(prev[jj][i], pexp[jj], rowE[i] - 2 * HX_TOP);
          if (FULL || ok[i]) *reinterpret_cast<f32x4*>(crow[i] + 32 * (s - 1) + 16 * jj) = v;
        }
      } else if constexpr (m < 6) {
        nexp[m - 4] = *reinterpret_cast<const int4*>(bexp + 32 * s + 16 * (m - 4) + 4 * g);
      } else if constexpr (m - 6 < T) {
        if constexpr (HD) {
          const int c = wave + 4 * (m - 6);
          const int q = c & 1, h = c >> 1, jj = h >= T ? 1 : 0, t = h - jj * T;
          const char* src = img + ((int64_t)t * NP + q) * img_piece + (int64_t)(32 * (s + 2) + 16 * jj) * 64;
          __builtin_amdgcn_global_load_lds((gptr_t)(src + lane * 16), (lptr_t)(dst + c * 1024), 16, 0, 0);
        }
      }
    };
    constexpr int NMEM = 6 + T, PER = (NMEM + T - 1) / T;         // memory instructions per k-tile
    ldb(b0, 0);
    bx_for<T>([&](auto tc) {
      constexpr int t = decltype(tc)::value;
      if constexpr ((t & 1) == 0) { if constexpr (t + 1 < T) ldb(b1, t + 1); mma(b0, tc); }
      else                        { if constexpr (t + 1 < T) ldb(b0, t + 1); mma(b1, tc); }
      bx_for<PER>([&](auto kc) { mem_op(std::integral_constant<int, t * PER + decltype(kc)::value>{}); });
    });
    // (the order the scheduler must keep: per k-tile the fragment reads of the next tile, 12 MFMAs, PER memory instructions)
    __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
    bx_for<T>([&](auto tc) {
      if constexpr (decltype(tc)::value + 1 < T) __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 12, 0);
      __builtin_amdgcn_sched_group_barrier(0x010, PER, 0);
    });
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      pexp[jj] = nexp[jj];
#pragma unroll
      for (int i = 0; i < 2; ++i) prev[jj][i] = acc[jj][i];
    }
  };
  using TT_ = std::true_type; using FF_ = std::false_type;
  // NS >= 4 (launcher: N >= 352).  Slot 0: nothing to store; slot 1: no stores are outstanding yet; the last two: no DMA
  slot_body(0, FF_{}, TT_{}, std::integral_constant<int, T>{});                       // (both first DMAs came from the prologue)
  slot_body(1, TT_{}, TT_{}, std::integral_constant<int, 2 + T>{});
  for (int s = 2; s < NS - 2; ++s) slot_body(s, TT_{}, TT_{}, std::integral_constant<int, 4 + 2 + T>{});
  slot_body(NS - 2, TT_{}, FF_{}, std::integral_constant<int, 4 + 2 + T>{});
  slot_body(NS - 1, TT_{}, FF_{}, std::integral_constant<int, 4 + 2>{});
  {                                                                // the last pair
#pragma unroll
    for (int jj = 0; jj < 2; ++jj)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const f32x4 v = hx_scale4(prev[jj][i], pexp[jj], rowE[i] - 2 * HX_TOP);
        if (FULL || ok[i]) *reinterpret_cast<f32x4*>(crow[i] + 32 * (NS - 1) + 16 * jj) = v;
      }
  }
}
__global__ __launch_bounds__(GEMM_THREADS, 2) void gemm_bx_astat_kernel(const GemmDev p) {
  __shared__ __attribute__((aligned(16))) char lds_dyn[AS_RING * 4 * AS_TMAX * 1024];      // 72 KB: two workgroups per CU
  int Mlim = p.M;
  if (p.m_dev) Mlim = min(Mlim, *p.m_dev);
  const int m0 = blockIdx.x * 128;
  if (m0 >= Mlim) return;
  const int T = (p.K[0] + BK - 1) / BK;                             // 1 .. AS_TMAX (launcher)
  const bool full = m0 + 128 <= Mlim;
  bx_for<AS_TMAX>([&](auto tc) {
    constexpr int TT = decltype(tc)::value + 1;
    if (T == TT) { if (full) bx_astat_body<true, TT>(p, lds_dyn); else bx_astat_body<false, TT>(p, lds_dyn); }
  });
}
// ---------------------------------------------------------------------------------------------
// The same contraction for SHORT operands (the layer-2 launches: a few thousand rows, where 128-row tiles leave most
// CUs idle and every workgroup is latency-bound): 32 rows x 176 columns per workgroup, wavefront w owns the column
// tiles w, w+4, w+8 of all 32 rows; two LDS buffers, ONE barrier per k-tile, and two register stages so that the
// global loads of k-tiles t+2 and t+3 are in flight while tile t is multiplied.  Pre-split B image only.
// NT = column tiles (of 16) per workgroup: 11 (the whole 176-column block of the image) or 4 - launches with a few dozen
// row tiles (layer 2 at C2: 80) put three times the workgroups on the chip, each staging a third of the image per k-tile.
template <int NT, int FMT>
__global__ __launch_bounds__(GEMM_THREADS, 2) void gemm_bx_skinny_kernel(const GemmDev p) {
  constexpr int NP = BxFmt<FMT>::NP;
  constexpr int SK_B_PIECE = NT * 16 * 64;                     // bytes of one piece of the staged B slice
  constexpr int SK_BUF_BYTES = NP * SK_A_PIECE + NP * SK_B_PIECE + SK_ROWS * 4;   // + the row exponents of the A tile (FMT 1)
  constexpr int NU = (NP * (SK_B_PIECE / 16) + 255) / 256;     // 16-byte units of the B slice per thread
  constexpr int NJW = (NT + 3) / 4;                            // column tiles per wavefront
  __shared__ __attribute__((aligned(16))) char lds[2 * SK_BUF_BYTES];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int m0 = blockIdx.x * SK_ROWS, n0 = blockIdx.y * (NT * 16);
  int Mlim = p.M;
  if (p.m_dev) Mlim = min(Mlim, *p.m_dev);
  if (m0 >= Mlim) return;
  const int T0 = (p.K[0] + BK - 1) / BK;
  const int T1 = (p.K[1] > 0 && p.A[1]) ? (p.K[1] + BK - 1) / BK : 0;     // optional second K-concatenated source
  const int T = T0 + T1;
  f32x4 acc[2][NJW];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int jj = 0; jj < NJW; ++jj) acc[i][jj] = f32x4{0.f, 0.f, 0.f, 0.f};

  // staging: one float4 of A (row tid >> 3, k quad tid & 7) and NU 16-byte units of the B image per thread and stage
  float4 a_st[2];
  f32x4 i_st[2][NU];
  const int a_r = tid >> 3, a_c4 = tid & 7;
  const bool a_ok = m0 + a_r < Mlim;
  int64_t ridx0 = a_ok ? m0 + a_r : 0, ridx1 = ridx0;
  if (a_ok && p.a_idx[0]) ridx0 = p.a_idx[0][m0 + a_r];
  if (a_ok && T1 > 0 && p.a_idx[1]) ridx1 = p.a_idx[1][m0 + a_r];
  const float* a_row0 = p.A[0] + ridx0 * p.lda[0];
  const float* a_row1 = T1 > 0 ? p.A[1] + ridx1 * p.lda[1] : a_row0;
  const float* safe = p.A[0];
  const char* img0 = reinterpret_cast<const char*>(p.b_img) + (int64_t)n0 * 64;
  const char* img1 = T1 > 0 ? reinterpret_cast<const char*>(p.b_img2) + (int64_t)n0 * 64 : img0;
  const int64_t img_piece = (int64_t)p.b_img_rows * 64;
  const int img_units_left = min(SK_B_PIECE / 16, (p.b_img_rows - n0) * 4);      // 16-byte units of this slice inside the image
  // FMT 1: exponents of the image rows behind the tiles of each image; the A rows' running exponents travel with the tile
  const int32_t* bexp0 = reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(p.b_img) + (int64_t)T0 * NP * img_piece);
  const int32_t* bexp1 = T1 > 0 ? reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(p.b_img2) + (int64_t)T1 * NP * img_piece) : bexp0;
  int stE = HX_EMIN;                   // staging side: running exponent of row a_r (the same in its 8 staging lanes)
  int accE[2] = {HX_EMIN, HX_EMIN};    // accumulator side: the exponent the sums of this lane's two rows are scaled with
  auto load_global = [&](int t, auto sc) {
    constexpr int st = decltype(sc)::value;
    const bool second = t >= T0;
    const int ts = second ? t - T0 : t;
    const int k = ts * BK + 4 * a_c4;
    a_st[st] = ld4<true>((second ? a_row1 : a_row0) + k, a_ok ? (second ? p.K[1] : p.K[0]) - k : 0, safe);
    const char* tile = (second ? img1 : img0) + (int64_t)ts * NP * img_piece;
    bx_for<NU>([&](auto uc) {
      constexpr int u = decltype(uc)::value;
      const int unit = min(tid + 256 * u, NP * (SK_B_PIECE / 16) - 1);
      const int q = unit / (SK_B_PIECE / 16);
      // the last 64-column slice of a 176-row image block is 48 rows: rows beyond the image are clamped (their columns are never stored)
      const int in_piece = min(unit - q * (SK_B_PIECE / 16), img_units_left - 1);
      i_st[st][u] = *reinterpret_cast<const f32x4*>(tile + q * img_piece + in_piece * 16);
    });
  };
  auto store_lds = [&](int buf, auto sc) {
    constexpr int st = decltype(sc)::value;
    char* As = lds + buf * SK_BUF_BYTES;
    char* Bs = As + NP * SK_A_PIECE;
    {
      // the row's maximum over this k-tile sits in 8 neighbouring lanes (4 values each): quad swaps + half-row mirror
      const float4 v = a_st[st];
      uint32_t m = __float_as_uint(fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
      m = max(m, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, 0xB1, 0xF, 0xF, false));     // quad_perm [1,0,3,2]
      m = max(m, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, 0x4E, 0xF, 0xF, false));     // quad_perm [2,3,0,1]
      m = max(m, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, 0x141, 0xF, 0xF, false));    // row_half_mirror
      { const int e = hx_exp_of_bits(m); if (e > stE) stE = min(e + HX_GROW, HX_EMAX); }      // (headroom: see bx_split_rows)
      const int off = a_r * 64 + (((a_c4 >> 1) ^ bx_swz(a_r)) << 4) + ((a_c4 & 1) << 3);
      uint2 oh, ol;
      hx_split4(v, HX_TOP - stE, oh, ol);
      *reinterpret_cast<uint2*>(As + off) = oh;
      *reinterpret_cast<uint2*>(As + SK_A_PIECE + off) = ol;
      if (a_c4 == 0) reinterpret_cast<int32_t*>(As + NP * SK_A_PIECE + NP * SK_B_PIECE)[a_r] = stE;
    }
    bx_for<NU>([&](auto uc) {
      constexpr int u = decltype(uc)::value;
      const int unit = tid + 256 * u;
      if (256 * (u + 1) <= NP * (SK_B_PIECE / 16) || unit < NP * (SK_B_PIECE / 16)) *reinterpret_cast<f32x4*>(Bs + unit * 16) = i_st[st][u];
    });
  };
  const int frag_off = r * 64 + ((g ^ bx_swz(r)) << 4);
  auto compute = [&](int buf, int t) {
    const char* As = lds + buf * SK_BUF_BYTES;
    const char* Bs = As + NP * SK_A_PIECE;
    if constexpr (FMT == 1) {
      const int32_t* Es = reinterpret_cast<const int32_t*>(Bs + NP * SK_B_PIECE);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int e = Es[16 * i + r];
        if (e > accE[i]) {                                     // the row's scale moved with this tile: the sums follow
#pragma unroll
          for (int jj = 0; jj < NJW; ++jj)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[i][jj][c] = __builtin_amdgcn_ldexpf(acc[i][jj][c], accE[i] - e);
          accE[i] = e;
        }
      }
      if (T1 > 0 && t == T0) {                                 // second source: from the first image's row scales to the second's
#pragma unroll
        for (int jj = 0; jj < NJW; ++jj) {
          const int col = min(n0 + 16 * min(wave + 4 * jj, NT - 1) + 4 * g, p.b_img_rows - 4);
          const int4 e1 = *reinterpret_cast<const int4*>(bexp0 + col), e2 = *reinterpret_cast<const int4*>(bexp1 + col);
          const int4 d = {e1.x - e2.x, e1.y - e2.y, e1.z - e2.z, e1.w - e2.w};
#pragma unroll
          for (int i = 0; i < 2; ++i) acc[i][jj] = hx_scale4(acc[i][jj], d, 0);
        }
      }
    }
    u32x4 a[2][NP], b[NJW][NP];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int q = 0; q < NP; ++q) a[i][q] = *reinterpret_cast<const u32x4*>(As + q * SK_A_PIECE + (16 * i) * 64 + frag_off);
#pragma unroll
    for (int jj = 0; jj < NJW; ++jj)
#pragma unroll
      for (int q = 0; q < NP; ++q) {
        const int j = min(wave + 4 * jj, NT - 1);             // NT = 11: wave 3 has no third tile, re-reads tile 10, result unused
        b[jj][q] = *reinterpret_cast<const u32x4*>(Bs + q * SK_B_PIECE + (16 * j) * 64 + frag_off);
      }
    {
      constexpr int PA[3] = {1, 0, 0}, PB[3] = {0, 1, 0};
#pragma unroll
      for (int t3 = 0; t3 < 3; ++t3)
#pragma unroll
        for (int jj = 0; jj < NJW; ++jj)
#pragma unroll
          for (int i = 0; i < 2; ++i)
            acc[i][jj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, b[jj][PB[t3]]), __builtin_bit_cast(f16x8, a[i][PA[t3]]), acc[i][jj], 0, 0, 0);
    }
  };
  using S0 = std::integral_constant<int, 0>;
  using S1 = std::integral_constant<int, 1>;
  load_global(0, S0{});
  if (T > 1) load_global(1, S1{});
  store_lds(0, S0{});
  if (T > 2) load_global(2, S0{});
  __syncthreads();
  for (int t = 0; t < T; t += 2) {
    if (t + 1 < T) {                       // tile t in buffer 0; stage 1 holds t+1, stage 0 has t+2 in flight
      store_lds(1, S1{});
      if (t + 3 < T) load_global(t + 3, S1{});
    }
    compute(0, t);
    __syncthreads();
    if (t + 1 >= T) break;
    if (t + 2 < T) {                       // tile t+1 in buffer 1; stage 0 holds t+2, stage 1 has t+3 in flight
      store_lds(0, S0{});
      if (t + 4 < T) load_global(t + 4, S0{});
    }
    compute(1, t + 1);
    __syncthreads();
  }
  float* Cb = p.C;
  const int64_t ldc = p.ldc;
  const bool n4 = bx_n4(p, Cb, ldc, p.bias);
  if (n4) {
    // every load of the epilogue in front of its first store (see bx_areg_body: a load may not pass a store that could alias
    // it, so the per-tile "exponents, addends, store" was a chain of load latencies)
    int colv[NJW]; bool okc[NJW];
    int4 ex[NJW]; float4 bs[NJW];
#pragma unroll
    for (int jj = 0; jj < NJW; ++jj) {
      const int j = wave + 4 * jj;
      const int col = n0 + 16 * j + 4 * g;
      okc[jj] = j < NT && col < p.N;
      colv[jj] = okc[jj] ? col : n0;                           // (n0 < N: a valid quad to read instead)
      ex[jj] = int4{0, 0, 0, 0}; bs[jj] = float4{0.f, 0.f, 0.f, 0.f};
      if constexpr (FMT == 1) ex[jj] = *reinterpret_cast<const int4*>(bexp1 + colv[jj]);
      if (p.bias) bs[jj] = *reinterpret_cast<const float4*>(p.bias + colv[jj]);
    }
    int rowv[2]; bool okr[2]; float rscale[2]; bool zero[2];
    float4 tc[2][NJW], ta[2][NJW], tr[2][NJW];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = m0 + 16 * i + r;
      okr[i] = row < Mlim;
      rowv[i] = okr[i] ? row : m0;
      rscale[i] = p.row_scale ? p.row_scale[(int64_t)rowv[i] * p.rs_ld] : 1.f;
      zero[i] = p.row_zero ? (p.row_zero[rowv[i]] != 0) : false;
      const float* addrow = p.add_src ? p.add_src + (int64_t)(p.add_idx ? p.add_idx[rowv[i]] : rowv[i]) * p.add_ld : nullptr;
#pragma unroll
      for (int jj = 0; jj < NJW; ++jj) {
        if (p.accumulate) tc[i][jj] = *reinterpret_cast<const float4*>(Cb + (int64_t)rowv[i] * ldc + colv[jj]);
        if (addrow) ta[i][jj] = *reinterpret_cast<const float4*>(addrow + colv[jj]);
        if (p.relu_src) tr[i][jj] = *reinterpret_cast<const float4*>(p.relu_src + (int64_t)rowv[i] * p.relu_ld + colv[jj]);
      }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int jj = 0; jj < NJW; ++jj) {
        f32x4 v = acc[i][jj];
        if constexpr (FMT == 1) v = hx_scale4(v, ex[jj], accE[i] - 2 * HX_TOP);
        if (p.accumulate) { v[0] += tc[i][jj].x; v[1] += tc[i][jj].y; v[2] += tc[i][jj].z; v[3] += tc[i][jj].w; }
        if (p.bias) { v[0] = fmaf(bs[jj].x, rscale[i], v[0]); v[1] = fmaf(bs[jj].y, rscale[i], v[1]); v[2] = fmaf(bs[jj].z, rscale[i], v[2]); v[3] = fmaf(bs[jj].w, rscale[i], v[3]); }
        if (p.add_src) { v[0] += ta[i][jj].x; v[1] += ta[i][jj].y; v[2] += ta[i][jj].z; v[3] += ta[i][jj].w; }
        if (zero[i]) v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (p.relu) { v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f); }
        if (p.relu_src) {
          v[0] = tr[i][jj].x > 0.f ? v[0] : 0.f; v[1] = tr[i][jj].y > 0.f ? v[1] : 0.f;
          v[2] = tr[i][jj].z > 0.f ? v[2] : 0.f; v[3] = tr[i][jj].w > 0.f ? v[3] : 0.f;
        }
        acc[i][jj] = v;
      }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int jj = 0; jj < NJW; ++jj)
        if (okr[i] && okc[jj]) *reinterpret_cast<f32x4*>(Cb + (int64_t)rowv[i] * ldc + colv[jj]) = acc[i][jj];
    return;
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = m0 + 16 * i + r;
    if (row >= Mlim) continue;
    const float rscale = p.row_scale ? p.row_scale[(int64_t)row * p.rs_ld] : 1.f;
    const bool zero = p.row_zero ? (p.row_zero[row] != 0) : false;
    const float* addrow = p.add_src ? p.add_src + (int64_t)(p.add_idx ? p.add_idx[row] : row) * p.add_ld : nullptr;
#pragma unroll
    for (int jj = 0; jj < NJW; ++jj) {
      const int j = wave + 4 * jj;
      const int col = n0 + 16 * j + 4 * g;
      if (j < NT && col < p.N) {
        f32x4 v = acc[i][jj];
        if constexpr (FMT == 1) v = hx_scale4(v, *reinterpret_cast<const int4*>(bexp1 + col), accE[i] - 2 * HX_TOP);
        bx_store4(p, Cb, ldc, p.bias, rscale, zero, n4, row, col, v, addrow);
      }
    }
  }
}

int gemm_bx_run(int form, dim3 grid, dim3 block, const GemmDev& d, hipStream_t stream) {
  switch (form) {
    case PFO_GEMM_FORM_SKINNY4: PFO_KLAUNCH((gemm_bx_skinny_kernel<4, 1>), grid, block, 0, stream, d); break;
    case PFO_GEMM_FORM_SKINNY11: PFO_KLAUNCH((gemm_bx_skinny_kernel<11, 1>), grid, block, 0, stream, d); break;
    case PFO_GEMM_FORM_ASTAT: PFO_KLAUNCH(gemm_bx_astat_kernel, grid, block, 0, stream, d); break;
    case PFO_GEMM_FORM_AREG8: PFO_KLAUNCH(gemm_bx_areg8_kernel<1>, grid, block, 0, stream, d); break;
    case PFO_GEMM_FORM_AREG: PFO_KLAUNCH(gemm_bx_areg_kernel<1>, grid, block, 0, stream, d); break;
  }
  PFO_LAUNCH_CHECK();
  return PFO_OK;
}
