// What FusedAdam queues in FRONT of the Adam kernel (misc.hip) when it clips or decays: the global L2 norm of the gradient
// (torch.nn.utils.clip_grad_norm_, norm_type 2) and the decoupled weight decay of torch.optim.AdamW, over the same element
// ranges of the flat buffers as pfo_adam_step_ranges.  Two launches, both memory-bound sweeps of at most the whole buffer:
//   grad_sumsq_kernel   : PFO_GRAD_NORM_PARTS workgroups, each sums the squares of a FIXED subset of the elements in fp64 - lane
//                         sums, a cross-lane butterfly inside the wavefront, one LDS slot per wavefront, one `partial` slot per
//                         workgroup.  No atomics: the subset and the order are functions of (lo, hi, PFO_GRAD_NORM_PARTS) alone.
//   grad_prestep_kernel : every workgroup folds the PFO_GRAD_NORM_PARTS slots in index order (the same bits everywhere - no
//                         second launch and no inter-workgroup hand-off to turn the partial sums into one coefficient), then
//                         scales its share of the gradient by the clip coefficient and of the parameters by the decay factor.
// Element -> lane mapping of one range [lo, hi), shared by both kernels: the elements in front of the first multiple of 4
// (at most 3) and behind the last whole group of 4 go to the first lanes of the grid one by one; the groups of 4 in between
// are dealt round robin over the grid's lanes, as one 16-byte access where the buffer's base is 16-byte aligned and as four
// 4-byte accesses in the same order where it is not.
#include "common.hpp"
#include <algorithm>
#include <cmath>

struct GradRanges { int64_t lo[PFO_ADAM_MAX_RANGES], hi[PFO_ADAM_MAX_RANGES]; int n; };

struct RangeCut { int64_t body, n_vec, tail; };      // [lo, body) singles, n_vec groups of 4 from body, [tail, hi) singles
__device__ __forceinline__ RangeCut cut_range(int64_t lo, int64_t hi) {
  RangeCut c;
  c.body = std::min<int64_t>(hi, (lo + 3) & ~(int64_t)3);
  c.n_vec = (hi - c.body) >> 2;
  c.tail = c.body + 4 * c.n_vec;
  return c;
}

template <bool VEC>
__device__ __forceinline__ float4 load4(const float* __restrict__ p) {
  if (VEC) return *reinterpret_cast<const float4*>(p);
  return make_float4(p[0], p[1], p[2], p[3]);
}
template <bool VEC>
__device__ __forceinline__ void store4(float* __restrict__ p, const float4 v) {
  if (VEC) { *reinterpret_cast<float4*>(p) = v; return; }
  p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
}

__device__ __forceinline__ double wave_sum_f64(double v) {      // xor butterfly: a + b == b + a, so every lane ends with the same bits
#pragma unroll
  for (int off = PFO_WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, PFO_WAVE);
  return v;
}

template <bool VEC>
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, const GradRanges r, double* __restrict__ partial,
                                                         int accumulate) {
  __shared__ double s_wave[256 / PFO_WAVE];
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x, T = (int64_t)gridDim.x * 256;
  double acc = 0.0;
  for (int q = 0; q < r.n; ++q) {
    const int64_t lo = r.lo[q], hi = r.hi[q];
    const RangeCut c = cut_range(lo, hi);
    if (lo + t < c.body) { const double x = (double)g[lo + t]; acc += x * x; }
    for (int64_t v = t; v < c.n_vec; v += T) {
      const float4 x = load4<VEC>(g + c.body + 4 * v);
      acc += (double)x.x * (double)x.x;
      acc += (double)x.y * (double)x.y;
      acc += (double)x.z * (double)x.z;
      acc += (double)x.w * (double)x.w;
    }
    if (c.tail + t < hi) { const double x = (double)g[c.tail + t]; acc += x * x; }
  }
  acc = wave_sum_f64(acc);
  if ((threadIdx.x & (PFO_WAVE - 1)) == 0) s_wave[threadIdx.x / PFO_WAVE] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = s_wave[0];
#pragma unroll
    for (int w = 1; w < 256 / PFO_WAVE; ++w) s += s_wave[w];
    partial[blockIdx.x] = accumulate ? partial[blockIdx.x] + s : s;
  }
}

// the host arrays into the kernel's argument block; the message of the refusal, or nullptr
static const char* fill_ranges(GradRanges& r, int32_t n_ranges, const int64_t* lo, const int64_t* hi, int64_t* longest) {
  if (n_ranges < 1 || n_ranges > PFO_ADAM_MAX_RANGES) return "bad range count";
  if (!lo || !hi) return "null range arrays";
  r.n = n_ranges;
  *longest = 0;
  for (int q = 0; q < n_ranges; ++q) {
    if (lo[q] < 0 || hi[q] < lo[q]) return "bad range";
    r.lo[q] = lo[q]; r.hi[q] = hi[q];
    *longest = std::max(*longest, hi[q] - lo[q]);
  }
  return nullptr;
}

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

extern "C" int pfo_grad_sumsq_ranges(const float* grad, int32_t n_ranges, const int64_t* lo, const int64_t* hi, double* partial,
                                     int32_t accumulate, void* stream) {
  PFO_REQUIRE(grad && partial, "null buffer");
  GradRanges r;
  int64_t longest;
  const char* bad = fill_ranges(r, n_ranges, lo, hi, &longest);
  PFO_REQUIRE(bad == nullptr, bad);
  // always the full grid: every slot is written, and the element -> slot mapping does not depend on the sizes
  if (aligned16(grad)) PFO_KLAUNCH(grad_sumsq_kernel<true>, dim3(PFO_GRAD_NORM_PARTS), dim3(256), 0, (hipStream_t)stream, grad, r, partial, (int)(accumulate != 0));
  else PFO_KLAUNCH(grad_sumsq_kernel<false>, dim3(PFO_GRAD_NORM_PARTS), dim3(256), 0, (hipStream_t)stream, grad, r, partial, (int)(accumulate != 0));
  PFO_LAUNCH_CHECK();
  return PFO_OK;
}

template <bool VEC, bool CLIP, bool DECAY>
__global__ __launch_bounds__(256) void grad_prestep_kernel(float* __restrict__ p, float* __restrict__ g, const GradRanges r,
                                                           const double* __restrict__ partial, float max_norm, float decay,
                                                           float* __restrict__ norm_out) {
  __shared__ float s_coef;
  float coef = 1.f;
  if (CLIP) {
    if (threadIdx.x == 0) {
      double s = 0.0;
      for (int i = 0; i < PFO_GRAD_NORM_PARTS; i += 8) {       // eight loads in flight, added in index order
        double x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = partial[i + j];
#pragma unroll
        for (int j = 0; j < 8; ++j) s += x[j];
      }
      const float total = (float)sqrt(s);
      const float c = max_norm / (total + 1e-6f);               // clip_grad_norm_: clamp(max_norm / (total + 1e-6), max=1); NaN stays
      s_coef = c > 1.f ? 1.f : c;
      if (blockIdx.x == 0) *norm_out = total;
    }
    __syncthreads();
    coef = s_coef;
  }
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x, T = (int64_t)gridDim.x * 256;
  for (int q = 0; q < r.n; ++q) {
    const int64_t lo = r.lo[q], hi = r.hi[q];
    const RangeCut c = cut_range(lo, hi);
    if (lo + t < c.body) {
      if (CLIP) g[lo + t] *= coef;
      if (DECAY) p[lo + t] *= decay;
    }
    for (int64_t v = t; v < c.n_vec; v += T) {
      const int64_t i = c.body + 4 * v;
      if (CLIP) {
        float4 x = load4<VEC>(g + i);
        x.x *= coef; x.y *= coef; x.z *= coef; x.w *= coef;
        store4<VEC>(g + i, x);
      }
      if (DECAY) {
        float4 x = load4<VEC>(p + i);
        x.x *= decay; x.y *= decay; x.z *= decay; x.w *= decay;
        store4<VEC>(p + i, x);
      }
    }
    if (c.tail + t < hi) {
      if (CLIP) g[c.tail + t] *= coef;
      if (DECAY) p[c.tail + t] *= decay;
    }
  }
}

template <bool VEC, bool CLIP, bool DECAY>
static void launch_prestep(int nb, hipStream_t s, float* p, float* g, const GradRanges& r, const double* partial, float max_norm, float decay,
                           float* norm_out) {
  const auto kernel = grad_prestep_kernel<VEC, CLIP, DECAY>;     // (a name without commas for the launch macro)
  PFO_KLAUNCH(kernel, dim3(nb), dim3(256), 0, s, p, g, r, partial, max_norm, decay, norm_out);
}

extern "C" int pfo_grad_prestep_ranges(float* param, float* grad, int32_t n_ranges, const int64_t* lo, const int64_t* hi,
                                       const double* partial, float max_norm, float decay, float* norm_out, void* stream) {
  const bool clip = max_norm > 0.f, decays = decay != 1.f;
  PFO_REQUIRE(!clip || (grad && partial && norm_out), "null buffer (clipping needs grad, partial and norm_out)");
  PFO_REQUIRE(!decays || param, "null buffer (decay needs param)");
  GradRanges r;
  int64_t longest;
  const char* bad = fill_ranges(r, n_ranges, lo, hi, &longest);
  PFO_REQUIRE(bad == nullptr, bad);
  if (!clip && !decays) return PFO_OK;
  const int nb = (int)std::min<int64_t>(2048, std::max<int64_t>(1, pfo_ceil_div(longest, 1024)));
  const bool vec = (!clip || aligned16(grad)) && (!decays || aligned16(param));
  hipStream_t s = (hipStream_t)stream;
  if (vec) {
    if (clip && decays) launch_prestep<true, true, true>(nb, s, param, grad, r, partial, max_norm, decay, norm_out);
    else if (clip) launch_prestep<true, true, false>(nb, s, param, grad, r, partial, max_norm, decay, norm_out);
    else launch_prestep<true, false, true>(nb, s, param, grad, r, partial, max_norm, decay, norm_out);
  } else {
    if (clip && decays) launch_prestep<false, true, true>(nb, s, param, grad, r, partial, max_norm, decay, norm_out);
    else if (clip) launch_prestep<false, true, false>(nb, s, param, grad, r, partial, max_norm, decay, norm_out);
    else launch_prestep<false, false, true>(nb, s, param, grad, r, partial, max_norm, decay, norm_out);
  }
  PFO_LAUNCH_CHECK();
  return PFO_OK;
}
