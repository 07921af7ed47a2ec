// The grouped weight gradients on the fp16 matrix cores (two fp16 pieces per element, three products per block: gemm_dev.hpp):
// the transposed-read tile, the grouped split-K kernel over it with its shader-clock pair, and the fold of the slabs.
#include "gemm_dev.hpp"
#include <string.h>

// ---------------------------------------------------------------------------------------------
// The weight gradient tile: C[m][n] = sum_k A[k][m] B[k][n], both operands k-major (k = instance row), so the
// MFMA fragments (8 consecutive k per lane) are TRANSPOSED reads of the staged tile: ds_read_b64_tr_b16 delivers a
// 4(k) x 16(m) block column-major, two of them make one 16x16x32 operand.  LDS image per piece: [k 0..31][row of
// 32-byte slots, one slot = 16 columns], A rows 256 B (8 slots), B rows 512 B (11 slots used); slot j of row k sits
// at slot (j + pi(k)) mod {8,16}, pi(k) = (k & 3) + 4 * ((k >> 3) & 1): the 8 rows a 32-lane half reads in one
// instruction ({0..3, 8..11} + 4h + 16 * half) land on 8 different 32-byte bank groups - conflict-free.
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));      // the type the transposed-read builtin is declared with (any 16-bit data)
#define TX_B_ROW 512
#define TX_B_PIECE (BK * TX_B_ROW)

__device__ __forceinline__ int tx_pi(int k) { return (k & 3) + ((k >> 1) & 4); }

// byte offset of columns col..col+3 of k-row `k` in a transposed-read image
__device__ __forceinline__ int tx_off(int row_bytes, int slot_mask, int k, int col) {
  return k * row_bytes + ((((col >> 4) + tx_pi(k)) & slot_mask) << 5) + ((col & 15) << 1);
}

__device__ __forceinline__ u32x4 tx_read(const char* piece, int row_bytes, int slot_mask, int slot, int g, int idx) {
  // lane (g, idx): block rows 8g + 4h + (idx >> 2), 8 bytes at column quad idx & 3
  typedef __attribute__((address_space(3))) bf16x4* lds_p;
  const int k0 = 8 * g + (idx >> 2), k1 = k0 + 4;
  const char* a0 = piece + k0 * row_bytes + (((slot + tx_pi(k0)) & slot_mask) << 5) + ((idx & 3) << 3);
  const char* a1 = piece + k1 * row_bytes + (((slot + tx_pi(k1)) & slot_mask) << 5) + ((idx & 3) << 3);
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_p)(a0));
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_p)(a1));
  return __builtin_bit_cast(u32x4, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// one 128 x 176 tile of a split-K weight gradient into its slab (the grouped launch below); VEC operands only
// Two fp16 pieces, three products, as everywhere: the contraction runs over the instance rows, so a per-row scale cannot be factored
// out; each OPERAND of the workgroup's K-slab takes ONE power-of-two scale instead - a running maximum over the k-tiles seen so
// far, with HX_GROW binades of headroom when it moves.  The maxima of the tile being staged are found while it waits in
// registers (per-wavefront maxima through eight LDS words, in front of the barrier that already separates the MFMAs of tile t
// from the staging of tile t+1); every thread derives the same two exponents from them, so the state lives in registers, the
// conversion takes a wave-uniform exponent, and when a scale moves the accumulators are multiplied by one exact power of two.
// Elements below 2^-16 of the slab's largest magnitude keep an absolute error of 2^-38 of it: norm-wise bound, as for the
// image kernels, now per slab and operand rather than per row.
__device__ __forceinline__ uint32_t tx_wave_max_u32(uint32_t u) {
  const auto a = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  u = max(a[0], a[1]);
  const auto b = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  u = max(b[0], b[1]);
  u = max(u, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)u, 0xB1, 0xF, 0xF, false));
  u = max(u, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)u, 0x4E, 0xF, 0xF, false));
  u = max(u, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)u, 0x124, 0xF, 0xF, false));
  return max(u, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)u, 0x128, 0xF, 0xF, false));
}
// W wavefronts per workgroup, 32 rows of the tile each: 4 (128 x 176, two workgroups per CU) or 8 (256 x 176, one per CU): the
// second form stages the B tile once per 256 rows instead of once per 128 - the launch's L2-level traffic (A once, B once per row
// tile) is what its time follows (profiles/r5_tn_stamps.txt).
template <int FMT, int W = 4>
__device__ __forceinline__ void gemm_tile_tn_bx(const GemmDev& p, int bx, int by, int split, char* lds) {
  constexpr int NP = BxFmt<FMT>::NP;
  constexpr int NT = 64 * W, TBM = 32 * W;                     // threads, rows of the tile
  constexpr int TXA_ROW = 2 * TBM, TXA_PIECE = BK * TXA_ROW, TXA_MASK = TBM / 16 - 1;
  constexpr int NA = BK * (TBM / 4) / NT, NB = (BK * 44 + NT - 1) / NT;      // float4 of the A / B tile per thread
  char* const As = lds;
  char* const Bs = lds + NP * TXA_PIECE;
  uint32_t* const wmax = reinterpret_cast<uint32_t*>(lds + NP * TXA_PIECE + NP * TX_B_PIECE);     // [W wavefronts: A | W: B]
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int m0 = bx * TBM, n0 = by * BN;
  int Kext = p.K[0];
  if (p.m_dev) Kext = min(Kext, *p.m_dev);
  const int chunk = p.dyn_chunk ? ((Kext + p.nsplit - 1) / p.nsplit + BK - 1) / BK * BK : p.split_chunk;
  const int kbeg = split * chunk;
  const int Ks = min(Kext, kbeg + chunk);
  const int wrow = 32 * wave;

  f32x4 acc[2][11];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 11; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int T = Ks > kbeg ? (Ks - kbeg + BK - 1) / BK : 0;
  const float* safe = p.A[0];
  const int64_t lda = p.lda[0], ldb = p.ldb[0];
  // per-thread invariants of the staging pass: which (k-row, column quad) of the tile each of the 4 + 6 float4 covers,
  // where it lands in LDS, and whether it holds the bias column
  float4 a_reg[NA], b_reg[NB];
  const float* a_ptr[NA];         // row kbeg + kr of A at this thread's columns; advanced by BK rows per tile
  int a_kr[NA], a_off[NA];
  bool a_col_ok[NA];
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const int f = tid + NT * i;
    a_kr[i] = f / (TBM / 4);
    const int mc = 4 * (f % (TBM / 4));
    a_col_ok[i] = m0 + mc < p.M;                        // M % 4 == 0 (VEC): a quad is all in or all out
    a_ptr[i] = p.A[0] + (int64_t)(kbeg + a_kr[i]) * lda + m0 + mc;
    a_off[i] = tx_off(TXA_ROW, TXA_MASK, a_kr[i], mc);
  }
  int b_kr[NB], b_off[NB], b_n[NB], b_bias_e[NB];
  bool b_live[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int f = tid + NT * i;
    b_kr[i] = f / 44;
    const int nc = 4 * (f - b_kr[i] * 44);
    b_live[i] = f < BK * 44;
    b_n[i] = n0 + nc;
    b_off[i] = tx_off(TX_B_ROW, 15, b_live[i] ? b_kr[i] : 0, nc);
    const int e = p.n_real - b_n[i];                     // bias column inside this quad?
    b_bias_e[i] = (p.n_real < p.N && e >= 0 && e < 4) ? e : -1;
  }

  // Branch-free staging loads: every lane loads from a clamped, always-valid address and the out-of-range values are
  // selected to zero afterwards (per-lane conditions around loads compile to exec-mask branch sequences: the first
  // version of this loop spent as many scalar as vector instructions).
  const int k_last = max(Ks - 1, 0);
  // gathered B rows: the row indices of tile t+1 are fetched while tile t is staged, so the row loads of a tile never
  // wait for an index load issued just before them
  int b_row_next[NB];
  auto fetch_rows = [&](int t) {
    const int k0 = kbeg + t * BK;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int kc = min(k0 + b_kr[i], k_last);
      b_row_next[i] = p.b_idx ? p.b_idx[kc] : kc;                       // wave-uniform test, unconditional load
    }
  };
  fetch_rows(0);
  auto load_tile = [&](int t) {
    const int k0 = kbeg + t * BK;
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const bool ok = a_col_ok[i] && (k0 + a_kr[i] < Ks);
      a_reg[i] = ld4<true>(a_ptr[i] + (int64_t)t * BK * lda, ok ? 4 : 0, safe);
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int k = k0 + b_kr[i];
      const bool ok = b_live[i] && k < Ks && b_n[i] < p.N;
      b_reg[i] = ld4<true>(p.B[0] + (int64_t)b_row_next[i] * ldb + b_n[i], ok ? p.n_real - b_n[i] : 0, safe);
      // bias column: dW's extra column accumulates sum_k dY[k][m]
      const int e = ok ? b_bias_e[i] : -1;
      b_reg[i].x = e == 0 ? 1.f : b_reg[i].x; b_reg[i].y = e == 1 ? 1.f : b_reg[i].y;
      b_reg[i].z = e == 2 ? 1.f : b_reg[i].z; b_reg[i].w = e == 3 ? 1.f : b_reg[i].w;
    }
    if (t + 1 < T) fetch_rows(t + 1);
  };
  int eA = HX_EMIN, eB = HX_EMIN;           // FMT 1: exponents of the two operands' scales (the same in every thread)
  // maxima of the tile in the staging registers -> one word per wavefront and operand (called in front of a barrier)
  auto publish_max = [&]() {
    float ma = 0.f, mb = 0.f;
#pragma unroll
    for (int i = 0; i < NA; ++i) ma = fmaxf(fmaxf(ma, fmaxf(fabsf(a_reg[i].x), fabsf(a_reg[i].y))), fmaxf(fabsf(a_reg[i].z), fabsf(a_reg[i].w)));
#pragma unroll
    for (int i = 0; i < NB; ++i) mb = fmaxf(fmaxf(mb, fmaxf(fabsf(b_reg[i].x), fabsf(b_reg[i].y))), fmaxf(fabsf(b_reg[i].z), fabsf(b_reg[i].w)));
    const uint32_t ua = tx_wave_max_u32(__float_as_uint(ma)), ub = tx_wave_max_u32(__float_as_uint(mb));
    if (lane == 0) { wmax[wave] = ua; wmax[W + wave] = ub; }
  };
  auto hstore = [&](char* base, int piece_bytes, int off, const float4 v, const int se) {
    uint2 oh, ol;
    hx_split4(v, se, oh, ol);
    *reinterpret_cast<uint2*>(base + off) = oh;
    *reinterpret_cast<uint2*>(base + piece_bytes + off) = ol;
  };
  auto store_tile = [&](bool first) {
    {
      uint32_t mwa = 0, mwb = 0;
#pragma unroll
      for (int q4 = 0; q4 < W / 4; ++q4) {
        const uint4 wa = *reinterpret_cast<const uint4*>(wmax + 4 * q4), wb = *reinterpret_cast<const uint4*>(wmax + W + 4 * q4);
        mwa = max(mwa, max(max(wa.x, wa.y), max(wa.z, wa.w))); mwb = max(mwb, max(max(wb.x, wb.y), max(wb.z, wb.w)));
      }
      const int ta = hx_exp_of_bits(mwa), tb = hx_exp_of_bits(mwb);
      const int nA = ta > eA ? min(ta + HX_GROW, HX_EMAX) : eA, nB = tb > eB ? min(tb + HX_GROW, HX_EMAX) : eB;
      if (nA != eA || nB != eB) {                              // a scale moves (the same decision in every thread): the sums follow
        if (!first) {
          const int d = (eA - nA) + (eB - nB);
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 11; ++j)
#pragma unroll
              for (int q = 0; q < 4; ++q) acc[i][j][q] = __builtin_amdgcn_ldexpf(acc[i][j][q], d);
        }
        eA = nA; eB = nB;
      }
      const int sa = HX_TOP - eA, sb = HX_TOP - eB;
#pragma unroll
      for (int i = 0; i < NA; ++i) hstore(As, TXA_PIECE, a_off[i], a_reg[i], sa);
#pragma unroll
      for (int i = 0; i < NB; ++i)
        if (b_live[i]) hstore(Bs, TX_B_PIECE, b_off[i], b_reg[i], sb);
    }
  };
  const int strips = __builtin_amdgcn_readfirstlane((m0 + wrow + 16 < p.M) ? 2 : ((m0 + wrow < p.M) ? 1 : 0));
  auto compute_tile = [&]() {
    u32x4 a[2][NP];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int q = 0; q < NP; ++q) a[i][q] = tx_read(As + q * TXA_PIECE, TXA_ROW, TXA_MASK, 2 * wave + i, g, r);
    auto ldb = [&](u32x4 (&b)[NP], int j) {
#pragma unroll
      for (int q = 0; q < NP; ++q) b[q] = tx_read(Bs + q * TX_B_PIECE, TX_B_ROW, 15, j, g, r);
    };
    // a wavefront whose strips lie beyond M skips their MFMAs (172-row gradients): `strips` is wave-uniform (an SGPR
    // after readfirstlane), so these are scalar branches, not exec-mask sequences
    auto mma = [&](const u32x4 (&b)[NP], int j) {
      if (strips >= 1) acc[0][j] = bx_mma<FMT>(a[0], b, acc[0][j]);
      if (strips >= 2) acc[1][j] = bx_mma<FMT>(a[1], b, acc[1][j]);
    };
    u32x4 b0[NP], b1[NP];                     // double-buffered B fragments: the reads of tile j+1 fly during the MFMAs of tile j
    ldb(b0, 0);
#pragma unroll
    for (int j = 0; j < 11; j += 2) {
      if (j + 1 < 11) ldb(b1, j + 1);
      mma(b0, j);
      if (j + 2 < 11) ldb(b0, j + 2);
      if (j + 1 < 11) mma(b1, j + 1);
    }
  };
  if (T > 0) {
    load_tile(0);
    if constexpr (FMT == 1) { publish_max(); __syncthreads(); }
    store_tile(true);
    __syncthreads();
    for (int t = 0; t < T; ++t) {
      const bool more = t + 1 < T;
      if (more) load_tile(t + 1);
      compute_tile();
      if constexpr (FMT == 1) { if (more) publish_max(); }
      __syncthreads();
      if (more) store_tile(false);
      __syncthreads();
    }
  }
  float* Cb = p.slab_base + (int64_t)split * (int64_t)p.M * p.N;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int row = m0 + wrow + 16 * i + 4 * g + reg;
      if (row >= p.M) continue;
#pragma unroll
      for (int j = 0; j < 11; ++j) {
        const int col = n0 + 16 * j + r;
        if (col < p.N) Cb[(int64_t)row * p.N + col] = FMT == 1 ? __builtin_amdgcn_ldexpf(acc[i][j][reg], eA + eB - 2 * HX_TOP) : acc[i][j][reg];
      }
    }
}

// ---------------------------------------------------------------------------------------------
// shader-clock pair of the grouped weight-gradient kernel (common.hpp pfo_clock_*); the device symbol and its reader share this file
__device__ unsigned long long g_gemm_clock[1][2];
int pfo_gemm_clock_read(double* out, int reset) {
  unsigned long long h[1][2];
  if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_gemm_clock), sizeof(h)) != hipSuccess) return PFO_ERR_HIP;
  out[0] = (double)h[0][0]; out[1] = (double)h[0][1];
  if (reset) { memset(h, 0, sizeof(h)); if (hipMemcpyToSymbol(HIP_SYMBOL(g_gemm_clock), h, sizeof(h)) != hipSuccess) return PFO_ERR_HIP; }
  return PFO_OK;
}
// the grouped launch (gemm_dev.hpp TnGroupDev) on the fp16 matrix cores (two pieces, three products, transposed LDS reads)
template <int FMT, int W = 4>
__global__ __launch_bounds__(64 * W, 2) void gemm_tn_group_bx_kernel(const TnGroupDev g) {
  __shared__ __attribute__((aligned(16))) char lds[BxFmt<FMT>::NP * (BK * 64 * W + TX_B_PIECE) + 64];
  const bool clk_on = blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < 64;
  PfoClockStamp clk;
  if (clk_on) clk = pfo_clock_begin();
  // Workgroups go to the XCDs round-robin by linear id.  All tiles of one K split read the same rows of A and B (a tile
  // takes 128 of A's columns and all of B's 172): with the (tile, split) grid the six tiles of dW1ovT's split sat on six
  // different L2s and B came from HBM six times (FETCH 188 MB per launch on average where the operands are 83 MB).  The
  // 1-D grid puts split s on XCD s & 7: id = (s / 8) * 8 * tiles + tile * 8 + (s & 7); a last group of fewer than eight
  // splits is laid out tile-major.
  int tile_id = blockIdx.x, split = blockIdx.y;
  if (g.xcd_map) {
    const int id = blockIdx.x, T = g.total_tiles;
    const int grp = id / (8 * T), loc = id - grp * 8 * T;
    const int in_grp = min(8, g.nsplit - 8 * grp);
    tile_id = loc / in_grp;
    split = 8 * grp + loc % in_grp;
  }
  int q = 0;
#pragma unroll
  for (int i = 1; i < TN_MAX_PROBLEMS; ++i)
    if (i < g.n && tile_id >= g.p[i].tile_begin) q = i;
  const TnProbDev& pr = g.p[q];
  const int t = tile_id - pr.tile_begin;
  GemmDev d;
  d.A[0] = pr.A; d.lda[0] = pr.lda; d.B[0] = pr.B; d.ldb[0] = pr.ldb; d.b_idx = pr.b_idx;
  d.K[0] = g.K; d.M = pr.M; d.N = pr.N; d.m_dev = g.k_dev;
  d.split_chunk = g.chunk;
  d.n_real = pr.N_real;
  d.slab_base = g.slabs + pr.slab_off;
  d.nsplit = g.nsplit;
  d.dyn_chunk = (g.k_dev != nullptr && g.nsplit > 1) ? 1 : 0;
  gemm_tile_tn_bx<FMT, W>(d, t / pr.tn, t % pr.tn, split, lds);
  if (clk_on && threadIdx.x == 0) pfo_clock_end(clk, g_gemm_clock[0]);
}
__global__ __launch_bounds__(256) void tn_group_reduce_kernel(const TnGroupDev g) {
  int K = g.K;
  if (g.k_dev) K = min(K, *g.k_dev);
  int chunk = g.chunk;
  if (g.k_dev && g.nsplit > 1) chunk = ((K + g.nsplit - 1) / g.nsplit + BK - 1) / BK * BK;   // same rule as gemm_tile
  int nz = chunk > 0 ? (K + chunk - 1) / chunk : 0;
  nz = min(nz, g.nsplit);
  for (int q = 0; q < g.n; ++q) {
    const TnProbDev& pr = g.p[q];
    const int64_t total = (int64_t)pr.M * pr.N;
    const float* slab = g.slabs + pr.slab_off;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
      // eight slab loads in flight per thread; the summation order (z ascending within four interleaved chains, then a
      // fixed tree) depends on nz only, so the result is reproducible
      float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
      int z = 0;
      for (; z + 8 <= nz; z += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = slab[(int64_t)(z + u) * total + e];
        s0 += v[0]; s1 += v[1]; s2 += v[2]; s3 += v[3];
        s0 += v[4]; s1 += v[5]; s2 += v[6]; s3 += v[7];
      }
      for (; z < nz; ++z) s0 += slab[(int64_t)z * total + e];
      const float s = (s0 + s1) + (s2 + s3);
      const int m = (int)(e / pr.N), n = (int)(e - (int64_t)m * pr.N);
      if (n < pr.N_real) {
        float* o = pr.C + (int64_t)m * pr.ldc + n;
        *o = pr.c_accumulate ? *o + s : s;
      } else {
        pr.bias_out[m] = pr.bias_accumulate ? pr.bias_out[m] + s : s;
      }
    }
  }
}

int gemm_tn_group_bx_run(int form, dim3 grid, dim3 block, const TnGroupDev& g, hipStream_t stream) {
  if (form == PFO_GEMM_FORM_TN_BX8) PFO_KLAUNCH((gemm_tn_group_bx_kernel<1, 8>), grid, block, 0, stream, g);
  else PFO_KLAUNCH(gemm_tn_group_bx_kernel<1>, grid, block, 0, stream, g);
  PFO_LAUNCH_CHECK();
  return PFO_OK;
}
int tn_group_reduce_run(dim3 grid, const TnGroupDev& g, hipStream_t stream) {
  PFO_KLAUNCH(tn_group_reduce_kernel, grid, dim3(256), 0, stream, g);
  PFO_LAUNCH_CHECK();
  return PFO_OK;
}
