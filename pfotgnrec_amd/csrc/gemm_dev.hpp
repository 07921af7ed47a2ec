// What the contraction's translation units share (internal): gemm.hip, the dispatcher, is host code and holds no kernel; each
// kernel family has a file of its own (gemm_f32.hip, gemm_bx.hip, gemm_tn_bx.hip; gemm_fused.hip and bimg.hip use the split
// helpers).  Device helpers are header-only and __forceinline__: no relocatable device code.  A kernel template is launched
// from the file that defines it, through the launch functions declared at the end.
#pragma once
#include "gemm.hpp"
#include <type_traits>

typedef float f32x4 __attribute__((ext_vector_type(4)));

// the output tile of the 128-row kernels is BM x BN over k-tiles of BK; 176 = 11 * 16 (see gemm_f32.hip)
constexpr int BM = 128;
constexpr int BN = 176;
constexpr int BK = 32;
constexpr int GEMM_THREADS = 256;

// XCD-aware tile order of a (row tiles x column tiles) launch flattened into a 1-D grid: workgroups go to the XCDs round-robin
// by id, so id = (t / 8) * 8 * tiles_n + c * 8 + (t mod 8) puts every column tile c of row tile t on XCD t & 7 - the A rows
// the column tiles share come from HBM once and from that XCD's L2 for the others.  false: no such tile (the last group).
__device__ __forceinline__ bool xcd_tile(int id, int tiles_m, int tiles_n, int& tm, int& tn) {
  const int per = 8 * tiles_n, grp = id / per, r = id - grp * per;
  tn = r >> 3;
  tm = grp * 8 + (r & 7);
  return tm < tiles_m;
}
struct GemmDev {
  int xcd_tm, xcd_tn;              // > 0: 1-D grid in xcd_tile order (row tiles, column tiles); 0: (row tile, column tile) = blockIdx.(x, y)
  const float* A[2]; int64_t lda[2]; const int32_t* a_idx[2];
  const float* B[2]; int64_t ldb[2]; const int32_t* b_idx;
  int K[2];
  float* C; int64_t ldc;
  const float* bias; const float* row_scale; int64_t rs_ld; const uint8_t* row_zero;
  const float* relu_src; int64_t relu_ld;
  const float* add_src; int64_t add_ld; const int32_t* add_idx;
  int M, N; const int32_t* m_dev;
  int relu, accumulate;
  int nsplit; int split_chunk;     // k-major split-K
  int64_t a_bs[2], b_bs[2], c_bs, bias_bs, rs_bs;
  int n_real;                      // columns of B that exist in memory; column n_real (if < N) is the bias column
  float* slab_base;                // split-K: this problem's slab region
  int dyn_chunk;                   // split-K chunk = f(device-side K) instead of split_chunk
  const void* b_img; int b_img_rows;   // pre-split image of B (source 0) and its padded row count
  const void* b_img2;                  // ... of the second K-concatenated source (same padded row count)
};

static inline bool aligned4(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// four consecutive floats of which `nv` lie inside the matrix; `safe` is any valid 16-byte aligned address,
// loaded instead of an out-of-range one so that the load itself needs no branch
template <bool VEC>
__device__ __forceinline__ float4 ld4(const float* p, int nv, const float* safe) {
  if (VEC) {
    const float4 v = *reinterpret_cast<const float4*>(nv > 0 ? p : safe);
    return nv > 0 ? v : float4{0.f, 0.f, 0.f, 0.f};
  } else {
    float4 r;
    r.x = nv > 0 ? p[0] : 0.f;
    r.y = nv > 1 ? p[1] : 0.f;
    r.z = nv > 2 ? p[2] : 0.f;
    r.w = nv > 3 ? p[3] : 0.f;
    return r;
  }
}

// ---------------------------------------------------------------------------------------------
// fp32 contraction on the 16-bit matrix cores by a split of every operand element into pieces (the format follows below).
// LDS image per piece: [row][32 halves] = 64-byte rows, 16-byte k-chunks XOR-swizzled with f(row >> 2) = {0,3,2,1} so that
// every ds_read_b128 fragment read covers all 64 banks exactly once.
template <int N, typename F, int I = 0>
__device__ __forceinline__ void bx_for(F&& f) {
  if constexpr (I < N) { f(std::integral_constant<int, I>{}); bx_for<N, F, I + 1>(static_cast<F&&>(f)); }
}
__device__ __forceinline__ int bx_swz(int row) { return (4 - ((row >> 2) & 3)) & 3; }   // {0,3,2,1}

// ---------------------------------------------------------------------------------------------
// The split format (the only one; FMT = 1 in the kernels' template arguments): every fp32 operand element is the sum of TWO fp16
// pieces of its value times a power of two, x * 2^s = h + l with h = fp16(x 2^s), l = fp16(x 2^s - h) (22 significant bits),
// and a 16x16x32 block takes THREE v_mfma_f32_16x16x32_f16 (h.l + l.h + h.h).  fp16 has 5 exponent bits, so the power of
// two is chosen per ROW of each operand, from the row's largest magnitude, so that the largest scaled value lies in
// [2^12, 2^15) (weight rows at the top, activation rows with HX_GROW binades of headroom): elements down to 2^-16 of their
// row's maximum keep all 22 bits, smaller ones an absolute error of 2^-38 of the row maximum - far below the rounding of an
// fp32 accumulation, but a NORM-wise bound, not a component-wise one.  Weight images carry the exponent of each image row behind the tiles (bimg_h_kernel); activation
// rows are scaled by the consuming kernel from a RUNNING maximum over the k-tiles it has seen: when a later tile holds a larger
// value the row's accumulators are multiplied by the (exact) power of two between the old and the new scale, the way an online
// softmax rescales its sums.  Powers of two throughout: scaling and unscaling are exact.
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
#define HX_EMIN 1             // clamp of the biased exponent of a row maximum: rows of zeros and denormals scale like 2^-126
#define HX_EMAX 254
#define HX_TOP 141            // a row whose exponent is E is scaled by 2^(HX_TOP - E): maximum in [2^14, 2^15)
#define HX_GROW 2             // binades of headroom a row takes when its running maximum outgrows its scale (see bx_split_rows)
// Every pre-split image and every kernel that reads one uses this format.  FMT stays a template parameter of those kernels
// (their symbols carry it); 1 is its only value.
template <int FMT> struct BxFmt;
template <> struct BxFmt<1> { static constexpr int NP = 2; };
__device__ __forceinline__ int hx_exp_of(float m) {           // biased exponent of |m| (m >= 0), clamped
  return min(max((int)(__float_as_uint(m) >> 23), HX_EMIN), HX_EMAX);
}
__device__ __forceinline__ int hx_exp_of_bits(uint32_t b) { return min(max((int)(b >> 23), HX_EMIN), HX_EMAX); }
// maximum over the four lanes r, r + 16, r + 32, r + 48 (the four k-groups of one fragment row), in every one of them: two
// lane-swap VALU instructions (gfx950), no LDS round trip.  Bits of non-negative floats order like unsigned integers.
__device__ __forceinline__ uint32_t hx_max_over_g(uint32_t u) {
  const auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  u = max(a[0], a[1]);
  const auto b = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return max(b[0], b[1]);
}
__device__ __forceinline__ float hx_absmax8(const float4 a, const float4 b) {
  return fmaxf(fmaxf(fmaxf(fabsf(a.x), fabsf(a.y)), fmaxf(fabsf(a.z), fabsf(a.w))),
               fmaxf(fmaxf(fabsf(b.x), fabsf(b.y)), fmaxf(fabsf(b.z), fabsf(b.w))));
}
// four values times 2^se -> the two fp16 pieces, packed two per dword (element e in the low half of dword e/2)
__device__ __forceinline__ void hx_split4(const float4 v, int se, uint2& oh, uint2& ol) {
  const f32x2 p0 = {__builtin_amdgcn_ldexpf(v.x, se), __builtin_amdgcn_ldexpf(v.y, se)};
  const f32x2 p1 = {__builtin_amdgcn_ldexpf(v.z, se), __builtin_amdgcn_ldexpf(v.w, se)};
  const f16x2 h0 = __builtin_convertvector(p0, f16x2), h1 = __builtin_convertvector(p1, f16x2);
  const f16x2 l0 = __builtin_convertvector(p0 - __builtin_convertvector(h0, f32x2), f16x2);   // residual exact in fp32
  const f16x2 l1 = __builtin_convertvector(p1 - __builtin_convertvector(h1, f32x2), f16x2);
  oh = uint2{__builtin_bit_cast(uint32_t, h0), __builtin_bit_cast(uint32_t, h1)};
  ol = uint2{__builtin_bit_cast(uint32_t, l0), __builtin_bit_cast(uint32_t, l1)};
}
// the products of one 16x16x32 block, smallest terms first; x = the operand whose rows become accumulator COLUMNS (first MFMA
// operand), y = the other one.  Pieces: hi | lo (fp16)
template <int FMT>
__device__ __forceinline__ f32x4 bx_mma(const u32x4 (&x)[BxFmt<FMT>::NP], const u32x4 (&y)[BxFmt<FMT>::NP], f32x4 c) {
#define BXM(q, w) c = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, x[q]), __builtin_bit_cast(f16x8, y[w]), c, 0, 0, 0)
  BXM(0, 1); BXM(1, 0); BXM(0, 0);
#undef BXM
  return c;
}
// product Q of bx_mma's list alone (two accumulators interleaved: a dependent MFMA waits for its predecessor's result)
template <int FMT, int Q>
__device__ __forceinline__ f32x4 bx_mma_q(const u32x4 (&x)[BxFmt<FMT>::NP], const u32x4 (&y)[BxFmt<FMT>::NP], f32x4 c) {
  constexpr int qx[3] = {0, 1, 0}, qy[3] = {1, 0, 0};
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, x[qx[Q]]), __builtin_bit_cast(f16x8, y[qy[Q]]), c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 hx_scale4(const f32x4 a, const int4 e, int base) {          // a[c] * 2^(base + e[c])
  return f32x4{__builtin_amdgcn_ldexpf(a[0], base + e.x), __builtin_amdgcn_ldexpf(a[1], base + e.y),
               __builtin_amdgcn_ldexpf(a[2], base + e.z), __builtin_amdgcn_ldexpf(a[3], base + e.w)};
}

// The A fragments of one k-tile from the raw rows a lane holds ([strip][half]: 8 consecutive k of one row per strip).  Keeps
// the running row scale (rowE) and moves the row's accumulators when a larger value arrives.
template <int FMT, int NJ, int S = 2>
__device__ __forceinline__ void bx_split_rows(const float4 (&a_raw)[S][2], u32x4 (&a)[S][BxFmt<FMT>::NP], int (&rowE)[S], f32x4 (&acc)[S][NJ],
                                              const bool first) {
#pragma unroll
  for (int i = 0; i < S; ++i) {
    {
      // the row's maximum over this k-tile: 8 values here, the other 24 in the lanes 16 / 32 / 48 further on
      const int e = hx_exp_of_bits(hx_max_over_g(__float_as_uint(hx_absmax8(a_raw[i][0], a_raw[i][1]))));
      if (e > rowE[i]) {                                     // a larger value than any before: the sums so far move to the new scale
        // HX_GROW binades of headroom with every move (a maximum that creeps up does not move the row at every tile); on the
        // first tile the sums are still zero and nothing has to move
        const int en = min(e + HX_GROW, HX_EMAX);
        if (!first) {
          const int d = rowE[i] - en;
#pragma unroll
          for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[i][j][c] = __builtin_amdgcn_ldexpf(acc[i][j][c], d);
        }
        rowE[i] = en;
      }
      const int se = HX_TOP - rowE[i];
      uint2 h0, l0, h1, l1;
      hx_split4(a_raw[i][0], se, h0, l0);
      hx_split4(a_raw[i][1], se, h1, l1);
      a[i][0] = u32x4{h0.x, h0.y, h1.x, h1.y};
      a[i][1] = u32x4{l0.x, l0.y, l1.x, l1.y};
    }
  }
}

// epilogue of the operand-swapped image kernels: four consecutive columns col..col+3 of one output row
__device__ __forceinline__ void bx_store4(const GemmDev& p, float* Cb, int64_t ldc, const float* bias, float rscale, bool zero,
                                          bool n4, int row, int col, const f32x4 a, const float* addrow = nullptr) {
  float v[4] = {a[0], a[1], a[2], a[3]};
  float* cp = Cb + (int64_t)row * ldc + col;
  if (n4) {
    if (p.accumulate) { const float4 o = *reinterpret_cast<const float4*>(cp); v[0] += o.x; v[1] += o.y; v[2] += o.z; v[3] += o.w; }
    if (bias) {
      const float4 bv = *reinterpret_cast<const float4*>(bias + col);
      v[0] = fmaf(bv.x, rscale, v[0]); v[1] = fmaf(bv.y, rscale, v[1]); v[2] = fmaf(bv.z, rscale, v[2]); v[3] = fmaf(bv.w, rscale, v[3]);
    }
    if (addrow) { const float4 o = *reinterpret_cast<const float4*>(addrow + col); v[0] += o.x; v[1] += o.y; v[2] += o.z; v[3] += o.w; }
    if (zero) { v[0] = v[1] = v[2] = v[3] = 0.f; }
    if (p.relu) { v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f); }
    if (p.relu_src) {
      const float4 m = *reinterpret_cast<const float4*>(p.relu_src + (int64_t)row * p.relu_ld + col);
      v[0] = m.x > 0.f ? v[0] : 0.f; v[1] = m.y > 0.f ? v[1] : 0.f; v[2] = m.z > 0.f ? v[2] : 0.f; v[3] = m.w > 0.f ? v[3] : 0.f;
    }
    *reinterpret_cast<float4*>(cp) = float4{v[0], v[1], v[2], v[3]};
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (col + e >= p.N) continue;
      float x = v[e];
      if (p.accumulate) x += cp[e];
      if (bias) x = fmaf(bias[col + e], rscale, x);
      if (addrow) x += addrow[col + e];
      if (zero) x = 0.f;
      if (p.relu) x = fmaxf(x, 0.f);
      if (p.relu_src) x = (p.relu_src[(int64_t)row * p.relu_ld + col + e] > 0.f) ? x : 0.f;
      cp[e] = x;
    }
  }
}
__device__ __forceinline__ bool bx_n4(const GemmDev& p, const float* Cb, int64_t ldc, const float* bias) {
  return (p.N & 3) == 0 && (ldc & 3) == 0 && (((uintptr_t)Cb) & 15) == 0 &&
         (!p.add_src || ((p.add_ld & 3) == 0 && (((uintptr_t)p.add_src) & 15) == 0)) &&
         (!p.relu_src || ((p.relu_ld & 3) == 0 && (((uintptr_t)p.relu_src) & 15) == 0)) && (!bias || (((uintptr_t)bias) & 15) == 0);
}

// limits of the image kernels that the plan (gemm.hip) tests before it names one
#define SK_ROWS 32            // rows of a gemm_bx_skinny_kernel workgroup
#define AS_TMAX 6             // gemm_bx_astat_kernel: k-tiles a wavefront keeps in registers ...
#define AS_NMAX 1024          // ... and the widest output it takes

// several small problems in one launch (gemm_multi_kernel)
#define MULTI_MAX PFO_GEMM_MULTI_MAX
struct MultiDev {
  GemmDev p[MULTI_MAX];
  int layout[MULTI_MAX];      // a_kmajor * 2 + b_kmajor
  int tile_begin[MULTI_MAX];  // first flattened tile of each problem
  int tm[MULTI_MAX], tn[MULTI_MAX];
  int n;
};
// Grouped weight gradients: every dW (+ bias gradient as one extra column) of a layer in ONE launch.
// All problems share the K extent (the layer's instance rows); K is split into `nsplit` chunks, each
// workgroup writes a partial slab tile, one grouped reduce folds the slabs into the gradient buffers.
#define TN_MAX_PROBLEMS 16
struct TnProbDev {
  const float* A; int64_t lda; const float* B; int64_t ldb; const int32_t* b_idx;
  float* C; int64_t ldc; float* bias_out; int bias_accumulate, c_accumulate;
  int M, N_real, N;          // N = N_real + (bias_out ? 1 : 0)
  int tile_begin, tn;        // first flattened tile, column tiles
  int64_t slab_off;          // floats
};
struct TnGroupDev {
  TnProbDev p[TN_MAX_PROBLEMS];
  int n, K, nsplit, chunk, total_tiles;
  int xcd_map;               // bx kernel, 1-D grid: every tile of one K split on the same XCD (split s on XCD s & 7)
  const int32_t* k_dev;
  float* slabs;
};

// The launch functions, one per dispatch site of gemm.hip: each takes the finished plan fields and the filled argument block
// and does PFO_KLAUNCH + PFO_LAUNCH_CHECK for the kernel instance they name - no argument checks, no plan decisions, no
// profiler calls (those bracket the call in gemm.hip).  `form` is a PFO_GEMM_FORM_* the file's kernels answer to.
int gemm_f32_run(int form, bool vec, bool a_km, bool b_km, dim3 grid, dim3 block, const GemmDev& d, hipStream_t stream);   // gemm_f32.hip
int gemm_multi_run(bool vec, dim3 grid, const MultiDev& g, hipStream_t stream);                                            // gemm_f32.hip
int gemm_tn_group_f32_run(dim3 grid, dim3 block, const TnGroupDev& g, hipStream_t stream);                                // gemm_f32.hip
int gemm_bx_run(int form, dim3 grid, dim3 block, const GemmDev& d, hipStream_t stream);                                   // gemm_bx.hip
int gemm_tn_group_bx_run(int form, dim3 grid, dim3 block, const TnGroupDev& g, hipStream_t stream);                       // gemm_tn_bx.hip
int tn_group_reduce_run(dim3 grid, const TnGroupDev& g, hipStream_t stream);                                              // gemm_tn_bx.hip
