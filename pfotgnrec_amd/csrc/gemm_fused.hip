// Contractions fused with what follows them, on the image kernels' staging and split helpers (gemm_dev.hpp): the lazy GRU with
// its gate math in the epilogue, and the message MLP's two layers (forward, backward) with the hidden tile kept on chip.
#include "gemm_dev.hpp"

// ---------------------------------------------------------------------------------------------
// The lazy GRU of the touched rows in ONE launch (memory_updater.py:18-61: torch.nn.GRUCell on [message | memory]): both
// contractions - message rows x W_ih^T (K = 3D + Ef) and memory rows x W_hh^T (K = D), K-concatenated - with the gate math in
// the epilogue, so the pre-activations gi / gh (2 x 3D floats per row) never go to HBM.  What makes that possible is the ORDER
// of the image rows (bimg_gate_row): a column block holds, for two groups of 16 hidden units, the four tiles r | z | n_i | n_h.
// In the operand-swapped accumulator layout lane (r, g) owns columns 4g .. 4g+3 of EVERY tile of row r: the r, z, n_i and n_h
// pre-activations of hidden units 16 q + 4g .. + 3 sit in one lane, in four accumulator tiles.  n_i takes only the message
// part and n_h only the memory part (n = tanh(n_i + r * n_h), torch GRUCell): their tiles skip the other source's k-tiles
// instead of multiplying zero rows, so no MFMA is spent that the two separate launches did not spend.
// Same staging as gemm_bx_areg_kernel: A rows straight to registers in fragment order and split there, the B image tile (128
// rows x 3 pieces = 24 KB) DMA'd into a double-buffered LDS image, one barrier per k-tile.
#define GF_NJ 8
#define GF_BN (GF_NJ * 16)
#define GF_B_PIECE (GF_BN * 64)
struct GruFusedDev {
  const float* msg_rows; int64_t ld_msg; int K0;
  const float* h_rows; int64_t ld_h; int K1;
  const void* img0; const void* img1; int img_rows;
  int xcd_tm, xcd_tn;              // as in GemmDev
  const float* b_ih; const float* b_hh;
  const uint8_t* hm; const int32_t* touched; const float* node_feat;
  float* upd_mem; float* h0_tab; float* gates;
  int D, M; const int32_t* m_dev;
  int gather;
};
int pfo_gru_img_rows(int D) { return (int)pfo_ceil_div(D, 32) * GF_BN; }
int64_t pfo_gru_img_bytes(int D, int K) { return (int64_t)pfo_ceil_div(K, 32) * 3 * pfo_gru_img_rows(D) * 64; }

__device__ __forceinline__ float gf_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-1.44269504088896340736f * x)); }
__device__ __forceinline__ float gf_tanh(float x) {
  const float e = __builtin_amdgcn_exp2f(-2.88539008177792681472f * fabsf(x));
  return copysignf((1.f - e) * __builtin_amdgcn_rcpf(1.f + e), x);
}

// PACKED_MSG (gather = 2): the state operands are the per-node tables as with gather = 1, the message rows are packed per
// touched row - an instance of its own, so that the two older forms keep their code as it was
template <int FMT, bool PACKED_MSG = false>
__global__ __launch_bounds__(GEMM_THREADS, 2) void gru_fused_kernel(const GruFusedDev p) {
  constexpr int NP = BxFmt<FMT>::NP;
  __shared__ __attribute__((aligned(16))) char lds[2 * NP * GF_B_PIECE];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  int tile_m = blockIdx.x, tile_n = blockIdx.y;
  if (p.xcd_tn > 0 && !xcd_tile(blockIdx.x, p.xcd_tm, p.xcd_tn, tile_m, tile_n)) return;
  const int m0 = tile_m * BM, n0 = tile_n * GF_BN;
  const int Mlim = min(p.M, p.m_dev ? *p.m_dev : p.M);
  if (m0 >= Mlim) return;
  const int wrow = 32 * wave;
  f32x4 acc[2][GF_NJ];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < GF_NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int T0 = (p.K0 + BK - 1) / BK, T1 = (p.K1 + BK - 1) / BK, T = T0 + T1;
  const float* safe = p.msg_rows;
  const int64_t img_piece = (int64_t)p.img_rows * 64;
  const float* a_row[2][2];
  bool a_ok[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int gm = m0 + wrow + 16 * i + r;
    a_ok[i] = gm < Mlim;
    int64_t ridx = a_ok[i] ? gm : 0;
    if constexpr (PACKED_MSG) a_row[0][i] = p.msg_rows + ridx * p.ld_msg + 8 * g;          // (before the row becomes a node id)
    if (p.gather) ridx = a_ok[i] ? p.touched[gm] : 0;          // straight from the per-node tables
    if constexpr (!PACKED_MSG) a_row[0][i] = p.msg_rows + ridx * p.ld_msg + 8 * g;
    a_row[1][i] = p.h_rows + ridx * p.ld_h + 8 * g;
  }
  const char* img[2] = {reinterpret_cast<const char*>(p.img0) + (int64_t)n0 * 64, reinterpret_cast<const char*>(p.img1) + (int64_t)n0 * 64};
  // FMT 1: exponents of the image rows of this block, behind the tiles of each image
  const int32_t* bexp[2] = {reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(p.img0) + (int64_t)T0 * NP * img_piece) + n0,
                            reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(p.img1) + (int64_t)T1 * NP * img_piece) + n0};
  // the rows of tile t live in register set t & 1 and are fetched TWO tiles ahead (as in bx_areg_body: with one set the loads of
  // tile t+1 had the 36 MFMAs of tile t to arrive in and every k-tile ended in a wait; 67-69 -> 60-65 us at C2)
  float4 a_raw[2][2][2];
  typedef __attribute__((address_space(1))) const void* gptr_t;
  typedef __attribute__((address_space(3))) void* lptr_t;
  auto load_a = [&](int t, auto setc) {
    constexpr int set = decltype(setc)::value;
    const int src = t < T0 ? 0 : 1;
    const int ts = src == 0 ? t : t - T0;
    const int k = ts * BK + 8 * g;
    const int Ks = src == 0 ? p.K0 : p.K1;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int h = 0; h < 2; ++h)
        a_raw[set][i][h] = ld4<true>(a_row[src][i] + ts * BK + 4 * h, a_ok[i] ? Ks - (k + 4 * h) : 0, safe);
  };
  auto load_b = [&](int t, int buf) {
    const int src = t < T0 ? 0 : 1;
    const int ts = src == 0 ? t : t - T0;
    const char* tile = img[src] + (int64_t)ts * NP * img_piece;
    char* Bs = lds + buf * NP * GF_B_PIECE;
    bx_for<2 * NP>([&](auto uc) {                              // NP pieces x 512 units of 16 bytes = 2 NP rounds of 256 threads
      constexpr int u = decltype(uc)::value;
      const int unit = tid + 256 * u;
      const int q = unit >> 9;                                 // 512 units per piece
      __builtin_amdgcn_global_load_lds((gptr_t)(tile + q * img_piece + (unit - (q << 9)) * 16),
                                       (lptr_t)(Bs + (64 * wave + 256 * u) * 16), 16, 0, 0);
    });
  };
  u32x4 a[2][NP];
  int rowE[2] = {HX_EMIN, HX_EMIN};
  auto split_a = [&](auto setc, bool first) { bx_split_rows<FMT, GF_NJ>(a_raw[decltype(setc)::value], a, rowE, acc, first); };
  const int frag_off = r * 64 + ((g ^ bx_swz(r)) << 4);
  // tiles that take source SRC: the message part feeds r, z, n_i (tiles 0 1 2 | 4 5 6), the memory part r, z, n_h (0 1 3 | 4 5 7)
  auto compute_tile = [&](int buf, auto src_c) {
    constexpr int SRC = decltype(src_c)::value;
    constexpr int act[6] = {0, 1, SRC == 0 ? 2 : 3, 4, 5, SRC == 0 ? 6 : 7};
    const char* Bs = lds + buf * NP * GF_B_PIECE;
    auto ldb = [&](u32x4 (&b)[NP], int j) {
#pragma unroll
      for (int q = 0; q < NP; ++q) b[q] = *reinterpret_cast<const u32x4*>(Bs + q * GF_B_PIECE + (16 * j) * 64 + frag_off);
    };
    auto mma = [&](const u32x4 (&b)[NP], int j) {
#pragma unroll
      for (int i = 0; i < 2; ++i) acc[i][j] = bx_mma<FMT>(b, a[i], acc[i][j]);
    };
    u32x4 b0[NP], b1[NP];
    ldb(b0, act[0]);
#pragma unroll
    for (int q = 0; q < 6; q += 2) {
      ldb(b1, act[q + 1]);
      mma(b0, act[q]);
      if (q + 2 < 6) ldb(b0, act[q + 2]);
      mma(b1, act[q + 1]);
    }
  };
  using C0 = std::integral_constant<int, 0>;
  using C1 = std::integral_constant<int, 1>;
  load_a(0, C0{});
  load_b(0, 0);
  if (T > 1) { load_a(1, C1{}); asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); }
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  split_a(C0{}, true);
  __syncthreads();
  auto step = [&](int t, auto curc) {
    constexpr int cur = decltype(curc)::value;                 // t & 1
    const bool more = t + 1 < T, more2 = t + 2 < T;
    if (more) load_b(t + 1, (t + 1) & 1);
    if (more2) load_a(t + 2, curc);                            // (the rows of tile t were split before this call)
    if constexpr (FMT == 1) {
      if (t == T0) {                                // the memory part: the r and z tiles move from W_ih's row scales to W_hh's
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
          for (int tt = 0; tt < 2; ++tt) {
            const int j = 4 * q + tt;
            const int4 e1 = *reinterpret_cast<const int4*>(bexp[0] + 16 * j + 4 * g);
            const int4 e2 = *reinterpret_cast<const int4*>(bexp[1] + 16 * j + 4 * g);
            const int4 d = {e1.x - e2.x, e1.y - e2.y, e1.z - e2.z, e1.w - e2.w};
#pragma unroll
            for (int i = 0; i < 2; ++i) acc[i][j] = hx_scale4(acc[i][j], d, 0);
          }
      }
    }
    if (t < T0) compute_tile(t & 1, std::integral_constant<int, 0>{}); else compute_tile(t & 1, std::integral_constant<int, 1>{});
    if (more) {
      // (the DMA is ordered only by the issuing wavefront's vmcnt + the barrier; the four row loads of tile t+2 were issued last)
      if (more2) asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      split_a(std::integral_constant<int, 1 - cur>{}, false);
    }
    __syncthreads();
  };
  for (int t = 0; t < T; t += 2) {
    step(t, C0{});
    if (t + 1 < T) step(t + 1, C1{});
  }
  // gates.  lane (r, g), strip i: row m0 + wrow + 16 i + r; group q: hidden units u0 .. u0 + 3, u0 = 32 by + 16 q + 4 g
  // Two passes: every load and the gate math of all four (strip, group) pairs first, the 24 stores after them - a load may not
  // pass a store that could alias it, so "load, compute, store" four times over was four load latencies one after the other.
  const int D = p.D;
  float hn_[2][2][4], h0_[2][2][4];
  bool live[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = m0 + wrow + 16 * i + r;
    const bool rok = row < Mlim;
    const int64_t id = p.touched[rok ? row : m0];
    const int64_t srow = p.gather ? id : (rok ? row : m0);     // row of the state operands (tables or packed copies)
    const bool has = p.hm[srow] != 0;
    if constexpr (FMT == 1) {                         // back to plain fp32: r, z and n_h carry W_hh's row scales, n_i W_ih's
#pragma unroll
      for (int j = 0; j < GF_NJ; ++j)
        acc[i][j] = hx_scale4(acc[i][j], *reinterpret_cast<const int4*>(bexp[(j & 3) == 2 ? 0 : 1] + 16 * j + 4 * g), rowE[i] - 2 * HX_TOP);
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int u0 = 32 * tile_n + 16 * q + 4 * g;
      live[i][q] = rok && u0 < D;                               // D % 4 == 0: a lane's four units are all inside or all outside
      const int uc = u0 < D ? u0 : 0;
      const float4 h4 = *reinterpret_cast<const float4*>(p.h_rows + srow * p.ld_h + uc);
      const float4 nf = *reinterpret_cast<const float4*>(p.node_feat + id * D + uc);
      const float hv[4] = {h4.x, h4.y, h4.z, h4.w}, nfv[4] = {nf.x, nf.y, nf.z, nf.w};
      float b_r[4], b_z[4], b_n[4], b_g[4];                     // (the bias vectors sit anywhere in the parameter buffer: scalar loads)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        b_r[e] = p.b_ih[uc + e] + p.b_hh[uc + e];
        b_z[e] = p.b_ih[D + uc + e] + p.b_hh[D + uc + e];
        b_n[e] = p.b_ih[2 * D + uc + e];
        b_g[e] = p.b_hh[2 * D + uc + e];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float pr = acc[i][4 * q + 0][e] + b_r[e];
        const float pz = acc[i][4 * q + 1][e] + b_z[e];
        const float pn = acc[i][4 * q + 2][e] + b_n[e];
        const float gh = acc[i][4 * q + 3][e] + b_g[e];
        const float rr = gf_sigmoid(pr);
        const float zz = gf_sigmoid(pz);
        const float nn = gf_tanh(pn + rr * gh);
        const float hn = has ? (1.f - zz) * nn + zz * hv[e] : hv[e];      // no pending message: the memory row is kept
        acc[i][4 * q + 0][e] = rr; acc[i][4 * q + 1][e] = zz; acc[i][4 * q + 2][e] = nn; acc[i][4 * q + 3][e] = gh;
        hn_[i][q][e] = hn; h0_[i][q][e] = hn + nfv[e];
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = m0 + wrow + 16 * i + r;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      if (!live[i][q]) continue;
      const int u0 = 32 * tile_n + 16 * q + 4 * g;
      *reinterpret_cast<float4*>(p.upd_mem + (int64_t)row * D + u0) = float4{hn_[i][q][0], hn_[i][q][1], hn_[i][q][2], hn_[i][q][3]};
      *reinterpret_cast<float4*>(p.h0_tab + (int64_t)row * D + u0) = float4{h0_[i][q][0], h0_[i][q][1], h0_[i][q][2], h0_[i][q][3]};
      float* gs = p.gates + (int64_t)row * 4 * D + u0;           // kept for the backward: r | z | n | gh_n
      *reinterpret_cast<f32x4*>(gs) = acc[i][4 * q + 0];
      *reinterpret_cast<f32x4*>(gs + D) = acc[i][4 * q + 1];
      *reinterpret_cast<f32x4*>(gs + 2 * D) = acc[i][4 * q + 2];
      *reinterpret_cast<f32x4*>(gs + 3 * D) = acc[i][4 * q + 3];
    }
  }
}

int pfo_gru_fused_launch(const PfoGruFused& f, hipStream_t stream) {
  PFO_REQUIRE(f.msg_rows && f.h_rows && f.img_ih && f.img_hh && f.b_ih && f.b_hh && f.hm && f.touched && f.node_feat && f.upd_mem &&
              f.h0_tab && f.gates, "null argument");
  PFO_REQUIRE(f.D > 0 && (f.D % 4) == 0 && f.K_msg > 0 && (f.K_msg % 4) == 0 && f.cap_rows > 0, "bad sizes");
  PFO_REQUIRE(f.gather >= 0 && f.gather <= 2, "gather must be 0, 1 or 2");
  PFO_REQUIRE(aligned4(f.msg_rows) && aligned4(f.h_rows) && aligned4(f.node_feat) && aligned4(f.upd_mem) && aligned4(f.h0_tab) &&
              aligned4(f.gates), "operands must be 16-byte aligned");
  GruFusedDev d;
  d.msg_rows = f.msg_rows; d.ld_msg = f.K_msg; d.K0 = f.K_msg; d.h_rows = f.h_rows; d.ld_h = f.D; d.K1 = f.D;
  d.img0 = f.img_ih; d.img1 = f.img_hh; d.img_rows = pfo_gru_img_rows(f.D);
  d.b_ih = f.b_ih; d.b_hh = f.b_hh; d.hm = f.hm; d.touched = f.touched; d.node_feat = f.node_feat;
  d.upd_mem = f.upd_mem; d.h0_tab = f.h0_tab; d.gates = f.gates; d.D = f.D; d.M = f.cap_rows; d.m_dev = f.n_rows;
  d.gather = f.gather;
  pfo_prof_begin(stream);
  const int tmr = (int)pfo_ceil_div(f.cap_rows, BM), tnc = (int)pfo_ceil_div(f.D, 32);
  dim3 grid((unsigned)tmr, (unsigned)tnc, 1);
  d.xcd_tm = d.xcd_tn = 0;
  if (tnc > 1) { d.xcd_tm = tmr; d.xcd_tn = tnc; grid = dim3((unsigned)(pfo_ceil_div(tmr, 8) * 8 * tnc), 1, 1); }
  if (f.gather == 2) PFO_KLAUNCH((gru_fused_kernel<1, true>), grid, dim3(GEMM_THREADS), 0, stream, d);
  else PFO_KLAUNCH(gru_fused_kernel<1>, grid, dim3(GEMM_THREADS), 0, stream, d);
  PFO_LAUNCH_CHECK();
  pfo_prof_end_dev(PFO_PROF_GRU_FUSED, 2.0 * 3 * f.D * ((double)f.K_msg + f.D), f.n_rows, f.cap_rows, stream);   // per-row FLOPs of the two contractions
  return PFO_OK;
}

// ---------------------------------------------------------------------------------------------
// The MLP message function (modules/message_function.py:13-26) of up to cap_rows rows in ONE launch:
//   hid = relu(raw W1^T + b1)  [rows, Hm],   out = hid W2^T + b2  [rows, Md]
// against the plain pre-split images of W1 [Hm, Mr] and W2 [Md, Hm] (pfo_bimg_launch).  A workgroup owns MM_ROWS = 64 rows, a
// wavefront 16 of them for BOTH layers, so the hidden row never leaves the lane that produced it: layer 1 runs in column
// blocks of 128 hidden units (eight accumulator tiles); in the operand-swapped accumulator layout lane (r, g) then holds
// hidden units 16 j + 4 g .. + 3 of row r for j = 0 .. 7, and two such tiles (j = 2 t', 2 t' + 1) ARE the A fragment of one
// 32-unit k-tile of layer 2 up to a permutation of the k slots - slot (g, e) stands for unit 4 g + e (e < 4) or 16 + 4 g +
// e - 4 - which a contraction does not see as long as the B fragment is read in the same permutation: two 8-byte LDS reads
// from chunks g / 2 and 2 + g / 2 of the image row where the plain form reads the 16 bytes of chunk g.  The hidden tile is
// split in registers like any A row (running row scale, bx_split_rows); it goes to HBM only when the caller asks for it.
// Staging as in gru_fused_kernel: A rows straight to registers in fragment order, the image tile (128 rows x 2 pieces = 16
// KB) by LDS-DMA into a double-buffered image, one barrier per k-tile.  Rows with hm == 0 are not read and give zeros.
#define MM_ROWS 64
struct MsgMlpDev {
  const float* raw; int64_t ld_raw; const int32_t* touched; const uint8_t* hm;
  const char* img1; const char* img2; int rows1, rows2;       // padded image rows
  const float* b1; const float* b2; float* hid; float* out;
  int Mr, Hm, Md, M; const int32_t* m_dev;
};
__global__ __launch_bounds__(GEMM_THREADS, 2) void msg_mlp_fwd_kernel(const MsgMlpDev p) {
  constexpr int FMT = 1, NP = BxFmt<FMT>::NP, NJ = GF_NJ;
  __shared__ __attribute__((aligned(16))) char lds[2 * NP * GF_B_PIECE];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int m0 = blockIdx.x * MM_ROWS, c0 = blockIdx.y * GF_BN;
  const int Mlim = min(p.M, p.m_dev ? *p.m_dev : p.M);
  if (m0 >= Mlim) return;
  const int row = m0 + 16 * wave + r;
  const bool rok = row < Mlim;
  const int64_t srow = rok ? (p.touched ? (int64_t)p.touched[row] : (int64_t)row) : 0;
  const bool has = rok && p.hm[srow] != 0;
  const float* a_ptr = p.raw + srow * p.ld_raw + 8 * g;
  const int T1 = (p.Mr + BK - 1) / BK, T2 = (p.Hm + BK - 1) / BK, NB = (p.Hm + GF_BN - 1) / GF_BN;
  const int64_t piece1 = (int64_t)p.rows1 * 64, piece2 = (int64_t)p.rows2 * 64;
  const int32_t* exps1 = reinterpret_cast<const int32_t*>(p.img1 + (int64_t)T1 * NP * piece1);
  const int32_t* exps2 = reinterpret_cast<const int32_t*>(p.img2 + (int64_t)T2 * NP * piece2);
  typedef __attribute__((address_space(1))) const void* gptr_t;
  typedef __attribute__((address_space(3))) void* lptr_t;
  // 128 image rows from row n0 of k-tile t into buffer buf; rows behind the image's padded end repeat its last row (their
  // columns are dropped in the epilogues)
  auto load_b = [&](const char* img, int64_t piece, int rows, int t, int n0, int buf) {
    const char* tile = img + (int64_t)t * NP * piece;
    char* Bs = lds + buf * NP * GF_B_PIECE;
    bx_for<2 * NP>([&](auto uc) {
      constexpr int u = decltype(uc)::value;
      const int unit = tid + 256 * u;
      const int q = unit >> 9, in = unit - (q << 9);
      const int srcrow = min(n0 + (in >> 2), rows - 1);
      __builtin_amdgcn_global_load_lds((gptr_t)(tile + q * piece + (int64_t)srcrow * 64 + (in & 3) * 16),
                                       (lptr_t)(Bs + (64 * wave + 256 * u) * 16), 16, 0, 0);
    });
  };
  const float* safe = p.raw;
  f32x4 acc2[1][NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) acc2[0][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  int rowE2[1] = {HX_EMIN};
  bool first2 = true;
  const int sw = bx_swz(r);
  const int frag_off = r * 64 + ((g ^ sw) << 4);
  const int frag_lo = r * 64 + (((g >> 1) ^ sw) << 4) + 8 * (g & 1);
  const int frag_hi = r * 64 + (((2 + (g >> 1)) ^ sw) << 4) + 8 * (g & 1);
  for (int nb = 0; nb < NB; ++nb) {
    const int n0 = nb * GF_BN;
    // ---- layer 1, hidden units n0 .. n0 + 127
    f32x4 acc1[1][NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc1[0][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    int rowE1[1] = {HX_EMIN};
    float4 a_raw[1][2];
    u32x4 a[1][NP];
    auto load_a = [&](int t) {
      const int k = t * BK + 8 * g;
#pragma unroll
      for (int h = 0; h < 2; ++h) a_raw[0][h] = ld4<true>(a_ptr + t * BK + 4 * h, has ? p.Mr - (k + 4 * h) : 0, safe);
    };
    load_b(p.img1, piece1, p.rows1, 0, n0, 0);
    load_a(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    bx_split_rows<FMT, NJ, 1>(a_raw, a, rowE1, acc1, true);
    __syncthreads();
    for (int t = 0; t < T1; ++t) {
      const bool more = t + 1 < T1;
      if (more) { load_b(p.img1, piece1, p.rows1, t + 1, n0, (t + 1) & 1); load_a(t + 1); }
      const char* Bs = lds + (t & 1) * NP * GF_B_PIECE;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        u32x4 b[NP];
#pragma unroll
        for (int q = 0; q < NP; ++q) b[q] = *reinterpret_cast<const u32x4*>(Bs + q * GF_B_PIECE + (16 * j) * 64 + frag_off);
        acc1[0][j] = bx_mma<FMT>(b, a[0], acc1[0][j]);
      }
      if (more) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        bx_split_rows<FMT, NJ, 1>(a_raw, a, rowE1, acc1, false);
      }
      __syncthreads();
    }
    // ---- hidden = relu(. + b1) in plain fp32, zero behind Hm and for rows without a message
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int cb = n0 + 16 * j + 4 * g;
      int4 e4 = {0, 0, 0, 0};
      if (cb < p.rows1) e4 = *reinterpret_cast<const int4*>(exps1 + cb);
      f32x4 v = hx_scale4(acc1[0][j], e4, rowE1[0] - 2 * HX_TOP);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = cb + e;
        v[e] = (has && c < p.Hm) ? fmaxf(v[e] + p.b1[c], 0.f) : 0.f;
      }
      acc1[0][j] = v;
      if (p.hid && rok && blockIdx.y == 0) {
        float* hp = p.hid + (int64_t)row * p.Hm + cb;
#pragma unroll
        for (int e = 0; e < 4; ++e) if (cb + e < p.Hm) hp[e] = v[e];
      }
    }
    // ---- layer 2 over these 128 hidden units: k-tiles 4 nb .. of W2's image
    const int nk = min(4, T2 - 4 * nb);
    load_b(p.img2, piece2, p.rows2, 4 * nb, c0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
      if (tt < nk) {
        if (tt + 1 < nk) load_b(p.img2, piece2, p.rows2, 4 * nb + tt + 1, c0, (tt + 1) & 1);
        float4 h_raw[1][2];
        h_raw[0][0] = float4{acc1[0][2 * tt][0], acc1[0][2 * tt][1], acc1[0][2 * tt][2], acc1[0][2 * tt][3]};
        h_raw[0][1] = float4{acc1[0][2 * tt + 1][0], acc1[0][2 * tt + 1][1], acc1[0][2 * tt + 1][2], acc1[0][2 * tt + 1][3]};
        u32x4 ah[1][NP];
        bx_split_rows<FMT, NJ, 1>(h_raw, ah, rowE2, acc2, first2);
        first2 = false;
        const char* Bs = lds + (tt & 1) * NP * GF_B_PIECE;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          u32x4 b[NP];
#pragma unroll
          for (int q = 0; q < NP; ++q) {
            const uint2 lo = *reinterpret_cast<const uint2*>(Bs + q * GF_B_PIECE + (16 * j) * 64 + frag_lo);
            const uint2 hi = *reinterpret_cast<const uint2*>(Bs + q * GF_B_PIECE + (16 * j) * 64 + frag_hi);
            b[q] = u32x4{lo.x, lo.y, hi.x, hi.y};
          }
          acc2[0][j] = bx_mma<FMT>(b, ah[0], acc2[0][j]);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
      }
    }
  }
  // ---- out = . + b2
  if (!rok) return;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int cb = c0 + 16 * j + 4 * g;
    if (cb >= p.Md) continue;                                   // Md % 4 == 0: a lane's four columns are all inside or all outside
    const int4 e4 = *reinterpret_cast<const int4*>(exps2 + cb);
    f32x4 v = hx_scale4(acc2[0][j], e4, rowE2[0] - 2 * HX_TOP);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = has ? v[e] + p.b2[cb + e] : 0.f;
    *reinterpret_cast<f32x4*>(p.out + (int64_t)row * p.Md + cb) = v;
  }
}

int pfo_msg_mlp_fwd_launch(const PfoMsgMlp& f, hipStream_t stream) {
  PFO_REQUIRE(f.raw && f.hm && f.img_w1 && f.img_w2 && f.b1 && f.b2 && f.msg_out, "pfo_msg_mlp_fwd_launch: null argument");
  PFO_REQUIRE(f.Mr > 0 && (f.Mr % 4) == 0 && f.Hm > 0 && f.Md > 0 && (f.Md % 4) == 0 && f.cap_rows > 0 && f.ld_raw >= f.Mr &&
              (f.ld_raw % 4) == 0, "pfo_msg_mlp_fwd_launch: bad sizes");
  PFO_REQUIRE(aligned4(f.raw) && aligned4(f.msg_out) && aligned4(f.img_w1) && aligned4(f.img_w2),
              "pfo_msg_mlp_fwd_launch: operands must be 16-byte aligned");
  MsgMlpDev d;
  d.raw = f.raw; d.ld_raw = f.ld_raw; d.touched = f.touched; d.hm = f.hm;
  d.img1 = reinterpret_cast<const char*>(f.img_w1); d.img2 = reinterpret_cast<const char*>(f.img_w2);
  d.rows1 = (int)pfo_align_up(f.Hm, BN); d.rows2 = (int)pfo_align_up(f.Md, BN);
  d.b1 = f.b1; d.b2 = f.b2; d.hid = f.hid; d.out = f.msg_out; d.Mr = f.Mr; d.Hm = f.Hm; d.Md = f.Md; d.M = f.cap_rows; d.m_dev = f.n_rows;
  const dim3 grid((unsigned)pfo_ceil_div(f.cap_rows, MM_ROWS), (unsigned)pfo_ceil_div(f.Md, GF_BN), 1);
  PFO_KLAUNCH(msg_mlp_fwd_kernel, grid, dim3(GEMM_THREADS), 0, stream, d);
  PFO_LAUNCH_CHECK();
  return PFO_OK;
}

// The data path of the MLP's backward in one launch, the mirror image of msg_mlp_fwd_kernel:
//   d m = dgi W_ih  [rows, Md]  (image of W_ih^T: Md rows, K = 3 D),   d hid = (d m W2) where hid > 0, else exactly 0  [rows, Hm]
//   (image of W2^T: Hm rows, K = Md).
// Md <= 128: d m is ONE column block of eight accumulator tiles, which stay in the lane and are the A fragments of the second
// contraction (same permuted read of the image as the forward); d hid leaves in column blocks of 128.  d m goes to HBM only
// when the caller asks for it (the weight gradients do).
struct MsgMlpBwdDev {
  const float* dgi; int K1; const float* hid;
  const char* img1; const char* img2; int rows1, rows2;
  float* d_m; float* d_hid;
  int Hm, Md, M; const int32_t* m_dev;
};
__global__ __launch_bounds__(GEMM_THREADS, 2) void msg_mlp_bwd_kernel(const MsgMlpBwdDev p) {
  constexpr int FMT = 1, NP = BxFmt<FMT>::NP, NJ = GF_NJ;
  __shared__ __attribute__((aligned(16))) char lds[2 * NP * GF_B_PIECE];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int m0 = blockIdx.x * MM_ROWS;
  const int Mlim = min(p.M, p.m_dev ? *p.m_dev : p.M);
  if (m0 >= Mlim) return;
  const int row = m0 + 16 * wave + r;
  const bool rok = row < Mlim;
  const float* a_ptr = p.dgi + (int64_t)(rok ? row : 0) * p.K1 + 8 * g;
  const int T1 = (p.K1 + BK - 1) / BK, T2 = (p.Md + BK - 1) / BK, NB = (p.Hm + GF_BN - 1) / GF_BN;
  const int64_t piece1 = (int64_t)p.rows1 * 64, piece2 = (int64_t)p.rows2 * 64;
  const int32_t* exps1 = reinterpret_cast<const int32_t*>(p.img1 + (int64_t)T1 * NP * piece1);
  const int32_t* exps2 = reinterpret_cast<const int32_t*>(p.img2 + (int64_t)T2 * NP * piece2);
  typedef __attribute__((address_space(1))) const void* gptr_t;
  typedef __attribute__((address_space(3))) void* lptr_t;
  auto load_b = [&](const char* img, int64_t piece, int rows, int t, int n0, int buf) {
    const char* tile = img + (int64_t)t * NP * piece;
    char* Bs = lds + buf * NP * GF_B_PIECE;
    bx_for<2 * NP>([&](auto uc) {
      constexpr int u = decltype(uc)::value;
      const int unit = tid + 256 * u;
      const int q = unit >> 9, in = unit - (q << 9);
      const int srcrow = min(n0 + (in >> 2), rows - 1);
      __builtin_amdgcn_global_load_lds((gptr_t)(tile + q * piece + (int64_t)srcrow * 64 + (in & 3) * 16),
                                       (lptr_t)(Bs + (64 * wave + 256 * u) * 16), 16, 0, 0);
    });
  };
  const float* safe = p.dgi;
  const int sw = bx_swz(r);
  const int frag_off = r * 64 + ((g ^ sw) << 4);
  const int frag_lo = r * 64 + (((g >> 1) ^ sw) << 4) + 8 * (g & 1);
  const int frag_hi = r * 64 + (((2 + (g >> 1)) ^ sw) << 4) + 8 * (g & 1);
  // ---- d m = dgi W_ih
  f32x4 acc1[1][NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) acc1[0][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  int rowE1[1] = {HX_EMIN};
  {
    float4 a_raw[1][2];
    u32x4 a[1][NP];
    auto load_a = [&](int t) {
      const int k = t * BK + 8 * g;
#pragma unroll
      for (int h = 0; h < 2; ++h) a_raw[0][h] = ld4<true>(a_ptr + t * BK + 4 * h, rok ? p.K1 - (k + 4 * h) : 0, safe);
    };
    load_b(p.img1, piece1, p.rows1, 0, 0, 0);
    load_a(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    bx_split_rows<FMT, NJ, 1>(a_raw, a, rowE1, acc1, true);
    __syncthreads();
    for (int t = 0; t < T1; ++t) {
      const bool more = t + 1 < T1;
      if (more) { load_b(p.img1, piece1, p.rows1, t + 1, 0, (t + 1) & 1); load_a(t + 1); }
      const char* Bs = lds + (t & 1) * NP * GF_B_PIECE;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        u32x4 b[NP];
#pragma unroll
        for (int q = 0; q < NP; ++q) b[q] = *reinterpret_cast<const u32x4*>(Bs + q * GF_B_PIECE + (16 * j) * 64 + frag_off);
        acc1[0][j] = bx_mma<FMT>(b, a[0], acc1[0][j]);
      }
      if (more) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        bx_split_rows<FMT, NJ, 1>(a_raw, a, rowE1, acc1, false);
      }
      __syncthreads();
    }
  }
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int cb = 16 * j + 4 * g;
    int4 e4 = {0, 0, 0, 0};
    if (cb < p.rows1) e4 = *reinterpret_cast<const int4*>(exps1 + cb);
    f32x4 v = hx_scale4(acc1[0][j], e4, rowE1[0] - 2 * HX_TOP);
    if (cb >= p.Md || !rok) v = f32x4{0.f, 0.f, 0.f, 0.f};         // Md % 4 == 0
    acc1[0][j] = v;
    if (p.d_m && rok && cb < p.Md) *reinterpret_cast<f32x4*>(p.d_m + (int64_t)row * p.Md + cb) = v;
  }
  // ---- d hid = (d m W2) (hid > 0), 128 hidden units at a time
  for (int nb = 0; nb < NB; ++nb) {
    const int n0 = nb * GF_BN;
    f32x4 acc2[1][NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc2[0][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    int rowE2[1] = {HX_EMIN};
    load_b(p.img2, piece2, p.rows2, 0, n0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
      if (tt < T2) {
        if (tt + 1 < T2) load_b(p.img2, piece2, p.rows2, tt + 1, n0, (tt + 1) & 1);
        float4 h_raw[1][2];
        h_raw[0][0] = float4{acc1[0][2 * tt][0], acc1[0][2 * tt][1], acc1[0][2 * tt][2], acc1[0][2 * tt][3]};
        h_raw[0][1] = float4{acc1[0][2 * tt + 1][0], acc1[0][2 * tt + 1][1], acc1[0][2 * tt + 1][2], acc1[0][2 * tt + 1][3]};
        u32x4 ah[1][NP];
        bx_split_rows<FMT, NJ, 1>(h_raw, ah, rowE2, acc2, tt == 0);
        const char* Bs = lds + (tt & 1) * NP * GF_B_PIECE;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          u32x4 b[NP];
#pragma unroll
          for (int q = 0; q < NP; ++q) {
            const uint2 lo = *reinterpret_cast<const uint2*>(Bs + q * GF_B_PIECE + (16 * j) * 64 + frag_lo);
            const uint2 hi = *reinterpret_cast<const uint2*>(Bs + q * GF_B_PIECE + (16 * j) * 64 + frag_hi);
            b[q] = u32x4{lo.x, lo.y, hi.x, hi.y};
          }
          acc2[0][j] = bx_mma<FMT>(b, ah[0], acc2[0][j]);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
      }
    }
    if (rok) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int cb = n0 + 16 * j + 4 * g;
        if (cb >= p.Hm) continue;
        const int4 e4 = *reinterpret_cast<const int4*>(exps2 + cb);  // (cb < Hm <= rows2, both multiples of 4 apart from Hm's tail)
        const f32x4 v = hx_scale4(acc2[0][j], e4, rowE2[0] - 2 * HX_TOP);
        const float* hp = p.hid + (int64_t)row * p.Hm + cb;
        float* dp = p.d_hid + (int64_t)row * p.Hm + cb;
#pragma unroll
        for (int e = 0; e < 4; ++e) if (cb + e < p.Hm) dp[e] = hp[e] > 0.f ? v[e] : 0.f;
      }
    }
  }
}

int pfo_msg_mlp_bwd_launch(const PfoMsgMlpBwd& f, hipStream_t stream) {
  PFO_REQUIRE(f.dgi && f.hid && f.img_wihT && f.img_w2T && f.d_hid, "pfo_msg_mlp_bwd_launch: null argument");
  PFO_REQUIRE(f.D3 > 0 && (f.D3 % 4) == 0 && f.Hm > 0 && f.Md > 0 && (f.Md % 4) == 0 && f.cap_rows > 0, "pfo_msg_mlp_bwd_launch: bad sizes");
  PFO_REQUIRE(f.Md <= GF_BN, "pfo_msg_mlp_bwd_launch: msg_dim beyond 128 takes the composed contractions");
  PFO_REQUIRE(aligned4(f.dgi) && aligned4(f.img_wihT) && aligned4(f.img_w2T) && (!f.d_m || aligned4(f.d_m)),
              "pfo_msg_mlp_bwd_launch: operands must be 16-byte aligned");
  MsgMlpBwdDev d;
  d.dgi = f.dgi; d.K1 = f.D3; d.hid = f.hid;
  d.img1 = reinterpret_cast<const char*>(f.img_wihT); d.img2 = reinterpret_cast<const char*>(f.img_w2T);
  d.rows1 = (int)pfo_align_up(f.Md, BN); d.rows2 = (int)pfo_align_up(f.Hm, BN);
  d.d_m = f.d_m; d.d_hid = f.d_hid; d.Hm = f.Hm; d.Md = f.Md; d.M = f.cap_rows; d.m_dev = f.n_rows;
  PFO_KLAUNCH(msg_mlp_bwd_kernel, dim3((unsigned)pfo_ceil_div(f.cap_rows, MM_ROWS)), dim3(GEMM_THREADS), 0, stream, d);
  PFO_LAUNCH_CHECK();
  return PFO_OK;
}
