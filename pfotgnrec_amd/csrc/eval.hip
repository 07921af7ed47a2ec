// Evaluation batch in one launch (evaluation.py:114-207): scores of the positive and the N candidate negatives, the positive's
// rank, recall / NDCG@{1,3,5}, the top-5 candidates in the canonical order and the change of annualised return and Sharpe ratio
// when the top-1/3/5 stocks join the user's portfolio, in-sample and out-of-sample.
//
// One workgroup of four wavefronts per interaction.
//   A  scores.  A row of 16 lanes takes one candidate's embedding row as 16-byte loads (D = 172 floats = 43 float4: three
//      per lane, the last one partly masked) and folds its 16 partial dot products with four row-local DPP adds; a workgroup
//      has 16 such rows and every row has four candidates' loads in flight per pass (64 candidates per workgroup pass, 12
//      dwordx4 loads per lane outstanding).  The source row stays in registers.  Scores go to LDS; emb is read once.
//   B  wavefront 0: rank = #{negatives scoring >= the positive}; five rounds of a wave-wide arg-max over (score, position) give
//      the head of the canonical order (stable ascending argsort reversed, SURVEY App. A-9: score descending, the LARGER
//      position first among equal scores).  Lanes r < n_ret then hold column r of the per-day log-return sums: the portfolio
//      rows first, the top-5 rows added one by one (the order np.mean(axis=0) adds the rows of np.concatenate([portfolio,
//      top-k]), evaluation.py:28-32), divided by the row count at k = 1, 3, 5.
//   C  eight lanes, one per daily-return series (table x {portfolio alone, k = 1, 3, 5}): mean and population standard
//      deviation in numpy's summation order (pfo_np_sum), return = mean * 251, sharpe = return / (std * sqrt(251)).
//   D  twelve lanes write new - old.
// fp64 throughout B-D, no contraction: the same operations in the same order as numpy, so the values are the reference's
// to the last bit wherever libm's log produced the tables on both sides.  No guards: a zero deviation gives inf / nan as numpy.
#include "common.hpp"

#pragma clang fp contract(off)

#define PFO_EVAL_THREADS 256
#define PFO_EVAL_ROWS 4          // candidates in flight per 16-lane row per pass
#define PFO_EVAL_MAX_RET 128
#define PFO_EVAL_MAX_CAND 12000  // scores of one interaction live in LDS (4 B each)

namespace {

__device__ __forceinline__ float dot4(const float4& a, const float4& b, float acc) {
  acc = fmaf(a.x, b.x, acc);
  acc = fmaf(a.y, b.y, acc);
  acc = fmaf(a.z, b.z, acc);
  return fmaf(a.w, b.w, acc);
}

__device__ __forceinline__ float4 load4_if(bool on, const float4* p) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (on) v = *p;
  return v;
}

// (score, position) of `o` comes before (s, c) in the canonical order; c < 0 = nothing held yet
__device__ __forceinline__ bool before(float os, int oc, float s, int c) {
  return oc >= 0 && (c < 0 || os > s || (os == s && oc > c));
}

// NJ float4 per lane cover a row of D <= 64 * NJ floats
template <int NJ>
__global__ __launch_bounds__(PFO_EVAL_THREADS) void eval_metrics_kernel(
    const float* __restrict__ emb, int64_t B, int D, int n_neg, const int32_t* __restrict__ cand,
    const int32_t* __restrict__ day_idx, const int32_t* __restrict__ port_idx, const int32_t* __restrict__ port_len,
    int port_stride, const double* __restrict__ ret_past, const double* __restrict__ ret_future, int n_days, int n_stocks,
    int n_ret, int upper_u, int64_t out_row0, int32_t* __restrict__ rank_out, float* __restrict__ hits, float* __restrict__ ndcg,
    int32_t* __restrict__ top5_pos, int32_t* __restrict__ top5_item, double* __restrict__ invest) {
  extern __shared__ double lds[];
  // daily[8][n_ret] | res[16] | scores[1 + n_neg]
  double* daily = lds;
  double* res = daily + 8 * n_ret;
  float* sc = reinterpret_cast<float*>(res + 16);
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x, g = tid >> 4, l = tid & 15;
  const int n_cand = 1 + n_neg;
  const int D4 = D >> 2;

  // ---- A: scores
  {
    const float4* srow = reinterpret_cast<const float4*>(emb + b * D);
    float4 sv[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) sv[j] = load4_if(l + 16 * j < D4, srow + l + 16 * j);
    for (int c0 = g; c0 < n_cand; c0 += 16 * PFO_EVAL_ROWS) {
      float4 v[PFO_EVAL_ROWS][NJ];
#pragma unroll
      for (int i = 0; i < PFO_EVAL_ROWS; ++i) {
        const int c = c0 + 16 * i;
        const bool on = c < n_cand;
        // candidate 0 is the destination's row, candidate c >= 1 the (c - 1)-th negative's
        const int64_t row = c == 0 ? B + b : 2 * B + b * n_neg + (c - 1);
        const float4* r = reinterpret_cast<const float4*>(emb + (on ? row : b) * D);
#pragma unroll
        for (int j = 0; j < NJ; ++j) v[i][j] = load4_if(on && l + 16 * j < D4, r + l + 16 * j);
      }
#pragma unroll
      for (int i = 0; i < PFO_EVAL_ROWS; ++i) {
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc = dot4(sv[j], v[i][j], acc);
        acc = pfo_row_sum(acc);
        const int c = c0 + 16 * i;
        if (l == 0 && c < n_cand) sc[c] = acc;
      }
    }
  }
  __syncthreads();

  // ---- B: rank, head of the canonical order, per-day portfolio sums
  const int plen = min(port_len[b], port_stride);
  if (tid < 64) {
    const int lane = tid;
    const float pos = sc[0];
    int rank = 0;
    for (int c0 = 1; c0 < n_cand; c0 += 64) {
      const int c = c0 + lane;
      rank += __popcll(__ballot(c < n_cand && sc[c] >= pos));
    }
    int top[5];
    float ps = 0.f;
    int pc = -1;                                                  // the previous pick; none before the first round
#pragma unroll
    for (int t = 0; t < 5; ++t) {
      float bs = 0.f;
      int bc = -1;
      for (int c = lane; c < n_cand; c += 64) {
        const float s = sc[c];
        const bool open = t == 0 || (pc >= 0 && (s < ps || (s == ps && c < pc)));   // behind the previous pick
        if (open && before(s, c, bs, bc)) { bs = s; bc = c; }
      }
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        const float os = __shfl_xor(bs, off, 64);
        const int oc = __shfl_xor(bc, off, 64);
        if (before(os, oc, bs, bc)) { bs = os; bc = oc; }
      }
      top[t] = bc;                                                // -1 once fewer than t + 1 candidates exist
      ps = bs;
      pc = bc;
    }
    int item[5];
#pragma unroll
    for (int t = 0; t < 5; ++t) item[t] = top[t] >= 0 ? cand[b * n_cand + top[t]] : -1;
    const int64_t o = out_row0 + b;
    if (lane == 0 && rank_out) rank_out[o] = rank;
    if (lane < 3) {
      const int k = 1 + 2 * lane;
      const bool hit = rank < k;
      if (hits) hits[o * 3 + lane] = hit ? 1.f : 0.f;                              // recall@k with one test item
      if (ndcg) ndcg[o * 3 + lane] = hit ? 1.f / log2f((float)rank + 2.f) : 0.f;  // idcg = 1
    }
    if (lane < 5) {
      const int tp = lane == 0 ? top[0] : lane == 1 ? top[1] : lane == 2 ? top[2] : lane == 3 ? top[3] : top[4];
      const int ti = lane == 0 ? item[0] : lane == 1 ? item[1] : lane == 2 ? item[2] : lane == 3 ? item[3] : item[4];
      if (top5_pos) top5_pos[o * 5 + lane] = tp;
      if (top5_item) top5_item[o * 5 + lane] = ti;
    }
    // a day or a stock outside the tables poisons the row's figures instead of reading out of bounds
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const int day = day_idx[b];
    const bool day_ok = day >= 0 && day < n_days;
    for (int tbl = 0; tbl < 2; ++tbl) {
      const double* base = (tbl == 0 ? ret_past : ret_future) + (int64_t)(day_ok ? day : 0) * n_stocks * n_ret;
      for (int r = lane; r < n_ret; r += 64) {
        double s = 0.0;
        int cnt = 0;
        for (int p = 0; p < plen; ++p) {
          const int st = port_idx[b * port_stride + p];
          s += (day_ok && st >= 0 && st < n_stocks) ? base[(int64_t)st * n_ret + r] : nan;
          ++cnt;
        }
        daily[(tbl * 4) * n_ret + r] = s / (double)cnt;           // (unused when the portfolio is empty)
#pragma unroll
        for (int t = 0; t < 5; ++t) {
          if (top[t] >= 0) {
            const int st = item[t] - upper_u - 1;
            s += (day_ok && st >= 0 && st < n_stocks) ? base[(int64_t)st * n_ret + r] : nan;
            ++cnt;
          }
          if ((t & 1) == 0) daily[(tbl * 4 + 1 + (t >> 1)) * n_ret + r] = s / (double)cnt;
        }
      }
    }
  }
  __syncthreads();

  // ---- C: return and Sharpe ratio of each series (evaluation.py:33-35, 160-172)
  if (tid < 8) {
    double ret = 0.0, sharpe = 0.0;                                // an empty portfolio alone: 0, 0 (evaluation.py:153-154)
    if ((tid & 3) != 0 || plen > 0) {
      double* x = daily + tid * n_ret;
      const double mean = pfo_np_sum(x, n_ret) / (double)n_ret;
      for (int i = 0; i < n_ret; ++i) {
        const double d = x[i] - mean;
        x[i] = d * d;
      }
      const double sd = sqrt(pfo_np_sum(x, n_ret) / (double)n_ret);
      ret = mean * 251.0;
      sharpe = ret / (sd * 15.84297951775486);                    // np.sqrt(251)
    }
    res[2 * tid] = ret;
    res[2 * tid + 1] = sharpe;
  }
  __syncthreads();

  // ---- D: (return@1,3,5 | sharpe@1,3,5) x (in-sample | out-of-sample)
  if (tid < 12 && invest) {
    const int tbl = tid / 6, kind = (tid % 6) / 3, ki = tid % 3;
    invest[(out_row0 + b) * 12 + tid] = res[2 * (tbl * 4 + 1 + ki) + kind] - res[2 * (tbl * 4) + kind];
  }
}

}  // namespace

extern "C" int pfo_eval_metrics(const float* emb, int64_t B, int32_t D, int32_t n_neg, const int32_t* cand,
                                const int32_t* day_idx, const int32_t* port_idx, const int32_t* port_len,
                                int32_t port_stride, const double* ret_past, const double* ret_future, int32_t n_days,
                                int32_t n_stocks, int32_t n_ret, int32_t upper_u, int64_t out_row0, int64_t out_rows,
                                int32_t* rank_out, float* hits_out, float* ndcg_out, int32_t* top5_pos, int32_t* top5_item,
                                double* invest_out, void* stream) {
  PFO_REQUIRE(B >= 0 && D > 0 && D % 4 == 0, "D must be a positive multiple of 4");
  PFO_REQUIRE(D <= 256, "D must be at most 256");
  PFO_REQUIRE(n_neg >= 1 && n_neg < PFO_EVAL_MAX_CAND, "n_neg must be in [1, 12000)");
  PFO_REQUIRE(n_ret >= 1 && n_ret <= PFO_EVAL_MAX_RET, "n_ret must be in [1, 128]");
  PFO_REQUIRE(n_days > 0 && n_stocks > 0 && port_stride >= 0, "bad table sizes");
  PFO_REQUIRE(out_row0 >= 0 && out_row0 + B <= out_rows, "rows [out_row0, out_row0 + B) exceed the output buffers");
  if (B == 0) return PFO_OK;
  PFO_REQUIRE(emb && cand && day_idx && port_len && ret_past && ret_future, "null input");
  PFO_REQUIRE(port_idx || port_stride == 0, "null port_idx");
  PFO_REQUIRE(((uintptr_t)emb & 15) == 0, "emb must be 16-byte aligned");
  const size_t shmem = (size_t)(8 * n_ret + 16) * sizeof(double) + (size_t)(1 + n_neg) * sizeof(float);
  const dim3 grid((unsigned)B), block(PFO_EVAL_THREADS);
  hipStream_t s = (hipStream_t)stream;
#define PFO_EVAL_LAUNCH(NJ)                                                                                              \
  PFO_KLAUNCH(eval_metrics_kernel<NJ>, grid, block, shmem, s, emb, B, (int)D, (int)n_neg, cand, day_idx, port_idx, port_len, \
              (int)port_stride, ret_past, ret_future, (int)n_days, (int)n_stocks, (int)n_ret, (int)upper_u, out_row0,    \
              rank_out, hits_out, ndcg_out, top5_pos, top5_item, invest_out)
  switch ((D + 63) / 64) {
    case 1: PFO_EVAL_LAUNCH(1); break;
    case 2: PFO_EVAL_LAUNCH(2); break;
    case 3: PFO_EVAL_LAUNCH(3); break;
    default: PFO_EVAL_LAUNCH(4); break;
  }
#undef PFO_EVAL_LAUNCH
  PFO_LAUNCH_CHECK();
  return PFO_OK;
}
