// Explanation query (TGN.explain): per root the DISTINCT nodes its embedding attends to, with the attention mass each one
// carries - read from what a forward-only pass leaves in the step workspace (the levels' neighbour ids, edge ids and dt, and the
// per-layer softmax weights attw).  Semantics: include/pfotgn.h (pfo_tgn_explain), DESIGN 4s.
//
// One root per workgroup.  Its P entries are the K sampled slots (hops 1) or the K * K two-hop paths q = j K + i (hops 2); an
// entry counts iff every neighbour id on it is non-zero.  The stages, each closed by a barrier every thread meets (all trip
// counts derive from kernel arguments and from two LDS words every thread reads behind a barrier):
//   weigh  : entry q gets its fp64 weight - the head mean of attw, for a path the rounded product of the two hops' means - and
//            the 64-bit key (node id << 32 | q); an entry that does not count gets the all-ones key and sorts behind the rest.
//   merge  : a bitonic sort of the keys in LDS.  The keys are distinct, so the sorted order IS the stable order by node: the
//            entries of a node are adjacent, q ascending.  Head flags, an inclusive scan, and every segment knows its start.
//   sum    : ONE lane per segment adds the weights sequentially in q order (what the host model does), counts the entries and
//            keeps the smallest dt with its edge id (strict <: among equal ages the lowest q).  No float atomics, no unordered
//            add: the same input gives the same bits on every run.  A thread holds up to four segments in registers, so the
//            per-segment rows may take the place of the per-entry ones after the next barrier: 24 bytes of LDS per entry,
//            96 KB for the 4096 paths of K = 64.
//   rank   : a bitonic sort of the segment indices by (weight descending, age ascending, node id ascending) - a total order,
//            the ids are distinct.
//   out    : every slot of every output row is written, padding included, by plain vector stores.
// fp64 WITHOUT contraction throughout: every product is rounded before it is added.
#include "explain.hpp"
#include <algorithm>

namespace {

constexpr int64_t EXP_MAX_GRID = 1 << 20;        // beyond that the workgroups stride over the roots
constexpr int EXP_PER_THREAD = 4;                // segments a thread may hold: blockDim.x * EXP_PER_THREAD >= padded entries
constexpr int EXP_MIN_BLOCK = 64;
constexpr unsigned long long EXP_NONE = ~0ull;   // the key of an entry that does not count

// p[k] = (sum over heads, ascending, of (double) attw[h, k]) / (double) H for a row attw [H, K]
__device__ __forceinline__ double exp_head_mean(const float* __restrict__ row, int H, int K, int k) {
#pragma clang fp contract(off)
  double s = 0.0;
  for (int h = 0; h < H; ++h) s += (double)row[h * K + k];
  return s / (double)H;
}
__device__ __forceinline__ double exp_mul(double a, double b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ double exp_add(double a, double b) {
#pragma clang fp contract(off)
  return a + b;
}

// a[0, n) ascending by `less`, n a power of two; every thread of the workgroup calls it; ends behind a barrier
template <class T, class Less>
__device__ __forceinline__ void exp_bitonic(T* a, int n, Less less) {
  for (int k = 2; k <= n; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int p = i ^ j;
        if (p > i) {
          const T x = a[i], y = a[p];
          if ((i & k) == 0 ? less(y, x) : less(x, y)) {
            a[i] = y;
            a[p] = x;
          }
        }
      }
      __syncthreads();
    }
}

__global__ void __launch_bounds__(1024) explain_kernel(const PfoExplain a, const int P, const int Ppad) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_explain[];
  __shared__ int s_segments, s_counting;
  // per entry ...
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(lds_explain);          // [Ppad]
  double* w = reinterpret_cast<double*>(lds_explain + (size_t)8 * Ppad);                  // [Ppad], by q
  int32_t* buf_x = reinterpret_cast<int32_t*>(lds_explain + (size_t)16 * Ppad);           // [Ppad]
  int32_t* buf_y = reinterpret_cast<int32_t*>(lds_explain + (size_t)20 * Ppad);           // [Ppad]
  // ... and, once the segments sit in registers, per segment in the same bytes
  float* seg_age = reinterpret_cast<float*>(lds_explain);                                 // [Ppad]
  int32_t* seg_eidx = reinterpret_cast<int32_t*>(lds_explain + (size_t)4 * Ppad);         // [Ppad]
  double* seg_w = w;                                                                      // [Ppad]
  int32_t* seg_node = buf_x;                                                              // [Ppad]
  uint16_t* seg_cnt = reinterpret_cast<uint16_t*>(buf_y);                                 // [Ppad] (a count is at most 4096)
  uint16_t* ord = seg_cnt + Ppad;                                                         // [Ppad]

  const int tid = threadIdx.x, nt = blockDim.x;
  const int K = a.K, H = a.H, m = a.m;
  const bool two = a.hops == 2;
  for (int64_t r = blockIdx.x; r < a.R; r += gridDim.x) {
    const int64_t e1 = r * K;                      // the root's first slot in the level-L tables
    const int64_t e2 = r * K * K;                  // its first path in the level-(L-1) tables: path q sits at e2 + q
    // ---- the tables the answer is made from, copied out as they are
    if (a.raw_nbr) {
      for (int c = tid; c < K; c += nt) {
        a.raw_nbr[e1 + c] = a.nbr[e1 + c];
        a.raw_dt[e1 + c] = a.dt[e1 + c];
        a.raw_eidx[e1 + c] = a.eidx[e1 + c];
      }
      for (int c = tid; c < H * K; c += nt) a.raw_w[e1 * H + c] = a.attw[e1 * H + c];
    }
    if (two && a.raw_nbr2) {
      for (int c = tid; c < K * K; c += nt) {
        a.raw_nbr2[e2 + c] = a.nbr2[e2 + c];
        a.raw_dt2[e2 + c] = a.dt2[e2 + c];
        a.raw_eidx2[e2 + c] = a.eidx2[e2 + c];
      }
      for (int c = tid; c < K * H * K; c += nt) a.raw_w2[e2 * H + c] = a.attw2[e2 * H + c];
    }
    // ---- weigh
    if (tid == 0) {
      s_segments = 0;
      s_counting = 0;
    }
    for (int q = tid; q < Ppad; q += nt) {
      unsigned long long key = EXP_NONE;
      double wq = 0.0;
      if (q < P) {
        const int j = two ? q / K : q;             // the first-hop slot
        const int32_t v1 = a.nbr[e1 + j];
        if (v1 != 0) {
          const double p1 = exp_head_mean(a.attw + e1 * H, H, K, j);
          if (!two) {
            key = ((unsigned long long)(uint32_t)v1 << 32) | (unsigned)q;
            wq = p1;
          } else {
            const int i = q - j * K;
            const int32_t v2 = a.nbr2[e2 + q];
            if (v2 != 0) {
              key = ((unsigned long long)(uint32_t)v2 << 32) | (unsigned)q;
              wq = exp_mul(p1, exp_head_mean(a.attw2 + (e1 + j) * H * K, H, K, i));
            }
          }
        }
      }
      keys[q] = key;
      w[q] = wq;
    }
    __syncthreads();
    // ---- merge
    exp_bitonic(keys, Ppad, [](unsigned long long x, unsigned long long y) { return x < y; });
    for (int p = tid; p < Ppad; p += nt) {
      const unsigned long long key = keys[p];
      const bool counting = key != EXP_NONE;
      buf_x[p] = (counting && (p == 0 || (keys[p - 1] >> 32) != (key >> 32))) ? 1 : 0;
      if (counting && (p == Ppad - 1 || keys[p + 1] == EXP_NONE)) s_counting = p + 1;     // (one thread at the most)
    }
    __syncthreads();
    int32_t* src = buf_x;
    int32_t* dst = buf_y;
    for (int off = 1; off < Ppad; off <<= 1) {     // inclusive scan of the head flags
      for (int p = tid; p < Ppad; p += nt) dst[p] = src[p] + (p >= off ? src[p - off] : 0);
      __syncthreads();
      int32_t* t = src; src = dst; dst = t;
    }
    for (int p = tid; p < Ppad; p += nt) {
      const bool head = src[p] != (p ? src[p - 1] : 0);
      if (head) dst[src[p] - 1] = p;               // segment -> its first sorted position
    }
    if (tid == 0) s_segments = src[Ppad - 1];
    __syncthreads();
    const int n_seg = s_segments, n_counting = s_counting;
    const int32_t* seg_start = dst;
    // ---- sum: one lane per segment, sequentially in q order
    double r_w[EXP_PER_THREAD];
    float r_age[EXP_PER_THREAD];
    int32_t r_eidx[EXP_PER_THREAD], r_node[EXP_PER_THREAD], r_cnt[EXP_PER_THREAD];
#pragma unroll
    for (int it = 0; it < EXP_PER_THREAD; ++it) {
      const int s = tid + it * nt;
      r_w[it] = 0.0; r_age[it] = 0.f; r_eidx[it] = -1; r_node[it] = -1; r_cnt[it] = 0;
      if (s < n_seg) {
        const int b = seg_start[s], e = s + 1 < n_seg ? seg_start[s + 1] : n_counting;
        double sum = 0.0;
        float best = 0.f;
        int32_t best_e = -1;
        for (int p = b; p < e; ++p) {
          const int q = (int)(keys[p] & 0xffffffffull);
          sum = exp_add(sum, w[q]);
          const float d = two ? a.dt2[e2 + q] : a.dt[e1 + q];
          if (p == b || d < best) {
            best = d;
            best_e = two ? a.eidx2[e2 + q] : a.eidx[e1 + q];
          }
        }
        r_w[it] = sum; r_age[it] = best; r_eidx[it] = best_e; r_cnt[it] = e - b;
        r_node[it] = (int32_t)(keys[b] >> 32);
      }
    }
    __syncthreads();                               // the per-entry rows are read no more: the segments take their place
#pragma unroll
    for (int it = 0; it < EXP_PER_THREAD; ++it) {
      const int s = tid + it * nt;
      if (s < n_seg) {
        seg_w[s] = r_w[it]; seg_age[s] = r_age[it]; seg_eidx[s] = r_eidx[it]; seg_node[s] = r_node[it];
        seg_cnt[s] = (uint16_t)r_cnt[it];
      }
    }
    int n_pad = 1;
    while (n_pad < n_seg) n_pad <<= 1;             // (n_seg <= Ppad, a power of two)
    for (int p = tid; p < n_pad; p += nt) ord[p] = (uint16_t)p;
    __syncthreads();
    // ---- rank
    exp_bitonic(ord, n_pad, [=](uint16_t x, uint16_t y) {
      if (x >= n_seg || y >= n_seg) return x < y;  // the filler indices sort behind the segments
      const double wx = seg_w[x], wy = seg_w[y];
      if (wx != wy) return wx > wy;
      const float ax = seg_age[x], ay = seg_age[y];
      if (ax != ay) return ax < ay;
      return seg_node[x] < seg_node[y];
    });
    // ---- out
    const int n_valid = std::min(m, n_seg);
    for (int p = tid; p < m; p += nt) {
      const int64_t o = r * m + p;
      const bool valid = p < n_valid;
      const int s = valid ? ord[p] : 0;
      a.node_out[o] = valid ? seg_node[s] : -1;
      a.weight_out[o] = valid ? seg_w[s] : 0.0;
      a.count_out[o] = valid ? (int32_t)seg_cnt[s] : 0;
      a.age_out[o] = valid ? seg_age[s] : __int_as_float(0x7fc00000);
      a.eidx_out[o] = valid ? seg_eidx[s] : -1;
    }
    if (tid == 0) a.n_valid_out[r] = n_valid;
    __syncthreads();                               // the next root rewrites the LDS rows
  }
}

}  // namespace

int pfo_explain_launch(const PfoExplain& a, hipStream_t s) {
  PFO_REQUIRE(a.R >= 1 && a.K >= 1 && a.K <= PFO_MAX_NEIGHBORS && a.H >= 1 && (a.hops == 1 || a.hops == 2) && a.m >= 1
                  && a.m <= PFO_EXPLAIN_MAX_WIDTH, "bad sizes");
  const int P = a.hops == 2 ? a.K * a.K : a.K;
  int Ppad = EXP_MIN_BLOCK;
  while (Ppad < P) Ppad <<= 1;
  const int block = std::max(EXP_MIN_BLOCK, Ppad / EXP_PER_THREAD);
  const size_t shmem = (size_t)24 * Ppad;
  if (shmem > 65536) {                             // (more than 64 KB of dynamic LDS has to be asked for)
    const hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void*>(&explain_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                              (int)shmem);
    if (ea != hipSuccess) {
      pfo_set_error("%s: %zu bytes of LDS refused: %s", __func__, shmem, hipGetErrorString(ea));
      return PFO_ERR_HIP;
    }
  }
  hipLaunchKernelGGL(explain_kernel, dim3((unsigned)std::min<int64_t>(a.R, EXP_MAX_GRID)), dim3(block), shmem, s, a, P, Ppad);
  PFO_LAUNCH_CHECK();
  return PFO_OK;
}
