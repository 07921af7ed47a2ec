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
#include "mv_value.hpp"

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

// The stages as device functions: eval_metrics_kernel is their composition, eval_metrics_mv_kernel puts its own ranking between
// stage A and the investment stages - so a score, a daily sum and a Sharpe ratio are each written down once.

// ---- A: the scores of interaction b's candidates into sc[1 + n_neg].  All threads; the caller's barrier follows.
// NJ float4 per lane cover a row of D <= 64 * NJ floats
template <int NJ>
__device__ __forceinline__ void eval_scores(const float* __restrict__ emb, int64_t B, int64_t b, int D, int n_neg, float* sc) {
  const int tid = threadIdx.x, g = tid >> 4, l = tid & 15;
  const int n_cand = 1 + n_neg;
  const int D4 = D >> 2;
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
}

// ---- what wavefront 0 writes of a ranked row o: the rank and what follows from it, the head of the order (top / item are
// the same in every lane, -1 in the empty slots)
__device__ __forceinline__ void eval_write_ranking(int lane, int64_t o, int rank, const int (&top)[5], const int (&item)[5],
                                                   int32_t* __restrict__ rank_out, float* __restrict__ hits, float* __restrict__ ndcg,
                                                   int32_t* __restrict__ top5_pos, int32_t* __restrict__ top5_item) {
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
}

// ---- B, second half: wavefront 0's lanes r < n_ret hold column r of the per-day log-return sums of interaction b - the
// portfolio rows first, the top-5 rows added one by one (a row with fewer picks adds what there is) - into daily[8][n_ret]
__device__ __forceinline__ void eval_daily_sums(double* daily, int lane, int64_t b, int plen, const int (&top)[5], const int (&item)[5],
                                                const int32_t* __restrict__ day_idx, const int32_t* __restrict__ port_idx,
                                                int port_stride, const double* __restrict__ ret_past,
                                                const double* __restrict__ ret_future, int n_days, int n_stocks, int n_ret, int upper_u) {
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
      daily[(tbl * 4) * n_ret + r] = s / (double)cnt;             // (unused when the portfolio is empty)
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

// ---- C and D, behind the barrier that ends B.  All threads.
__device__ __forceinline__ void eval_return_sharpe(double* daily, double* res, int plen, int n_ret, double* __restrict__ invest,
                                                   int64_t out_row0, int64_t b) {
  const int tid = threadIdx.x;
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
  const int tid = threadIdx.x;
  const int n_cand = 1 + n_neg;

  eval_scores<NJ>(emb, B, b, D, n_neg, sc);
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
    eval_write_ranking(lane, out_row0 + b, rank, top, item, rank_out, hits, ndcg, top5_pos, top5_item);
    eval_daily_sums(daily, lane, b, plen, top, item, day_idx, port_idx, port_stride, ret_past, ret_future, n_days, n_stocks, n_ret,
                    upper_u);
  }
  eval_return_sharpe(daily, res, plen, n_ret, invest, out_row0, b);
}

// ---------------------------------------------------------------------------------------------
// The same row ranked in a SERVED order (include/pfotgn.h, pfo_eval_metrics_mv): the rank fusion of main.py:243-289 (mode 0,
// what pfo_recommend_mv_topk serves) or the basket rounds of pfo_recommend_basket_topk with k = 5 (mode 1), then the investment
// stages above fed with that top-5.  One workgroup per interaction; a thread owns candidates tid, tid + 256, ...
//   A   eval_scores: pfo_eval_metrics's scores to the bit.
//   P   the pool: a candidate whose stock lies in the day's table gets mu and var (pfo_mv_mean / pfo_mv_var), the others mu = NaN,
//       which makes every y of theirs a NaN; then one pfo_mv_add_cov step per holding of the portfolio.  mu, var and the
//       covariance sum stay in LDS for the whole row: a later round adds one step per pick and re-derives nothing.
//   rounds (one in mode 0, up to five in mode 1) of
//   Y   y of the round from the three pieces (pfo_mv_finish - pfo_mv_value's operations in its order) into LDS, NaN = takes no part;
//   F   per owned candidate the two average-tie rank counts over LDS, four candidates per read (y is NaN from 1 + n_neg up to the
//       next multiple of 4; a score counts only where the y beside it is no NaN), blended into fused[] in LDS;
//   mode 0: the place of a candidate in the canonical order = the candidates before it, counted over fused[]; places below 5 fill
//       the top-5 slots, the positive's place is its rank.
//   mode 1: the pick = arg-max of (fused, position) over the thread, the wavefront (shuffles), the workgroup (four LDS slots); the
//       owner takes it out of the pool (mu = NaN), every thread adds the pick's covariance to its candidates' sums.
//   Then wavefront 0 reads the five slots and goes on as eval_metrics_kernel does.
// LDS: 44 bytes per candidate (score 4, y, fused, mu, var, sum 8 each) + 64 n_ret + 272; 96 KiB at 2048 candidates and n_ret 128.
// No atomics: counts are per-wavefront shuffles and four LDS slots.  Between two barriers every loop bound depends on n_neg,
// mode, the portfolio row and the pick alone - values all threads read from the same place.
struct EvalMvArgs {
  int mv_days, mv_stocks, mv_ret, mode;
  double gamma, lam;
  double* top5_fused;
  int32_t* n_adm;
  float* score_out;
  double *y_out, *fused_out;
};

// the canonical order over fused values: is (f, c) before the best so far (bf, bc)?  bc < 0: there is none yet
__device__ __forceinline__ bool mv_before(double f, int c, double bf, int bc) { return bc < 0 || f > bf || (f == bf && c > bc); }

template <int NJ>
__global__ __launch_bounds__(PFO_EVAL_THREADS) void eval_metrics_mv_kernel(
    const float* __restrict__ emb, int64_t B, int D, int n_neg, const int32_t* __restrict__ cand,
    const int32_t* __restrict__ day_idx, const int32_t* __restrict__ port_idx, const int32_t* __restrict__ port_len,
    int port_stride, const double* __restrict__ ret_past, const double* __restrict__ ret_future, int n_days, int n_stocks,
    int n_ret, int upper_u, int64_t out_row0, int32_t* __restrict__ rank_out, float* __restrict__ hits, float* __restrict__ ndcg,
    int32_t* __restrict__ top5_pos, int32_t* __restrict__ top5_item, double* __restrict__ invest,
    const double* __restrict__ ret_mv, const int32_t* __restrict__ mv_day_idx, const EvalMvArgs m) {
  extern __shared__ __attribute__((aligned(16))) double lds_mv[];
  const int n_cand = 1 + n_neg, IC = (n_cand + 3) & ~3, mv_ret = m.mv_ret;
  // every piece starts 16-byte aligned: the counts before yv and before sc are even
  double* daily = lds_mv;                                          // [8][n_ret]
  double* res = daily + 8 * n_ret;                                 // [16]
  double* yv = res + 16;                                           // [IC] y of the round
  double* fu = yv + IC;                                            // [IC] fused of the round
  double* mu = fu + IC;                                            // [IC] NaN: outside the pool
  double* var = mu + IC;                                           // [IC]
  double* ssum = var + IC;                                         // [IC] the covariances with the holdings so far
  double* wave_f = ssum + IC;                                      // [4] the best (fused, position) of each wavefront
  double* f5 = wave_f + 4;                                         // [6] fused of the top-5 (five in use)
  float* sc = reinterpret_cast<float*>(f5 + 6);                    // [IC]
  int* wave_c = reinterpret_cast<int*>(sc + IC);                   // [4]
  int* wave_n = wave_c + 4;                                        // [4] admissible candidates counted by each wavefront
  int* top5 = wave_n + 4;                                          // [8] the top-5 positions | the positive's rank | n_adm | -
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const double nan = __builtin_nan("");
  const double gamma = m.gamma, lam = m.lam;
  float* __restrict__ score_out = m.score_out;
  double *__restrict__ y_out = m.y_out, *__restrict__ fused_out = m.fused_out;
  const int32_t* cb = cand + b * n_cand;

  eval_scores<NJ>(emb, B, b, D, n_neg, sc);
  if (tid < 5) {
    top5[tid] = -1;
    f5[tid] = -__builtin_inf();
  }
  if (tid == 5) top5[5] = PFO_EVAL_RANK_NONE;
  __syncthreads();

  // ---- P: the pool and the portfolio's covariance sums
  const int day = mv_day_idx[b];
  const bool day_ok = day >= 0 && day < m.mv_days;                 // no day: nothing of ret_mv is read
  const double* dayp = ret_mv + (int64_t)(day_ok ? day : 0) * m.mv_stocks * mv_ret;
  const int plen_mv = (day_ok && port_idx && port_stride > 0) ? min(max(port_len[b], 0), port_stride) : 0;
  const double inv = pfo_mv_inv(mv_ret);
  for (int c = tid; c < n_cand; c += PFO_EVAL_THREADS) {
    if (score_out) score_out[b * n_cand + c] = sc[c];
    const int st = cb[c] - upper_u - 1;
    double mc = nan, vc = 0.0;
    if (day_ok && st >= 0 && st < m.mv_stocks) {
      const double* ri = dayp + (int64_t)st * mv_ret;
      mc = pfo_mv_mean(ri, mv_ret);
      vc = pfo_mv_var(ri, mc, mv_ret, inv);
    }
    mu[c] = mc;
    var[c] = vc;
    ssum[c] = 0.0;
  }
  // one more holding: row st of the day (in range) joins the sum of every pooled candidate this thread owns
  auto hold = [&](int st) {
    const double* rp = dayp + (int64_t)st * mv_ret;
    const double mp = pfo_mv_mean(rp, mv_ret);
    for (int c = tid; c < n_cand; c += PFO_EVAL_THREADS) {
      const double mc = mu[c];
      if (!(mc == mc)) continue;
      const double* ri = dayp + (int64_t)(cb[c] - upper_u - 1) * mv_ret;
      ssum[c] = pfo_mv_add_cov(ssum[c], ri, mc, rp, mp, mv_ret, inv);
    }
  };
  int n_hold = 0;
  for (int p = 0; p < plen_mv; ++p) {
    const int st = port_idx[b * port_stride + p];
    if ((unsigned)st >= (unsigned)m.mv_stocks) continue;
    ++n_hold;
    hold(st);
  }

  const int rounds = m.mode ? 5 : 1;
  bool pos_adm = false;                                            // the positive is in A(b)
  for (int rd = 0; rd < rounds; ++rd) {
    // ---- Y (a thread reads and writes its own candidates' pieces)
    for (int c = tid; c < IC; c += PFO_EVAL_THREADS) yv[c] = c < n_cand ? pfo_mv_finish(mu[c], gamma, var[c], ssum[c], n_hold) : nan;
    __syncthreads();
    if (rd == 0) pos_adm = yv[0] == yv[0];
    // ---- F
    double bf = 0.0;
    int bc = -1, mine = 0;
    for (int c = tid; c < IC; c += PFO_EVAL_THREADS) {
      const double yi = yv[c];
      double f = nan;
      if (yi == yi) {                                              // outside the pool, or a NaN y: out of this round
        ++mine;
        const float si = sc[c];
        int ly = 0, ey = 0, ls = 0, es = 0;
        const double2* y2 = reinterpret_cast<const double2*>(yv);
        const float4* s4 = reinterpret_cast<const float4*>(sc);
#pragma unroll 2
        for (int j = 0; j < IC; j += 4) {                          // (every comparison with a NaN is false)
          const double2 ya = y2[j >> 1], yb = y2[(j >> 1) + 1];
          const float4 sj = s4[j >> 2];
          const bool a0 = ya.x == ya.x, a1 = ya.y == ya.y, a2 = yb.x == yb.x, a3 = yb.y == yb.y;
          ly += (ya.x < yi) + (ya.y < yi) + (yb.x < yi) + (yb.y < yi);
          ey += (ya.x == yi) + (ya.y == yi) + (yb.x == yi) + (yb.y == yi);
          ls += (a0 && sj.x < si) + (a1 && sj.y < si) + (a2 && sj.z < si) + (a3 && sj.w < si);
          es += (a0 && sj.x == si) + (a1 && sj.y == si) + (a2 && sj.z == si) + (a3 && sj.w == si);   // (-0 == +0)
        }
        f = pfo_mv_blend(pfo_mv_avg_rank(ly, ey), pfo_mv_avg_rank(ls, es), lam);   // main.py:282-286
        if (f == f && mv_before(f, c, bf, bc)) {
          bf = f;
          bc = c;
        }
      }
      fu[c] = f;
      if (rd == 0 && c < n_cand) {
        if (y_out) y_out[b * n_cand + c] = yi;
        if (fused_out) fused_out[b * n_cand + c] = f;
      }
    }
    if (rd == 0) {                                                 // n_adm = |A(b)|
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) mine += __shfl_xor(mine, off, 64);
      if (lane == 0) wave_n[wave] = mine;
    }
    if (m.mode == 0) {
      __syncthreads();                                             // every fused value is in LDS
      if (tid == 0) top5[6] = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
      for (int c = tid; c < n_cand; c += PFO_EVAL_THREADS) {
        const double fi = fu[c];
        if (!(fi == fi)) continue;
        int place = 0;
        const double2* f2 = reinterpret_cast<const double2*>(fu);
#pragma unroll 2
        for (int j = 0; j < IC; j += 4) {
          const double2 fa = f2[j >> 1], fb = f2[(j >> 1) + 1];
          place += ((fa.x > fi) || (fa.x == fi && j > c)) + ((fa.y > fi) || (fa.y == fi && j + 1 > c)) +
                   ((fb.x > fi) || (fb.x == fi && j + 2 > c)) + ((fb.y > fi) || (fb.y == fi && j + 3 > c));
        }
        if (place < 5) {                                           // (places are distinct: the order is total)
          top5[place] = c;
          f5[place] = fi;
        }
        if (c == 0) top5[5] = place;
      }
      break;
    }
    // ---- the pick of round rd: the first of the canonical order
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const double of = __shfl_xor(bf, off, 64);
      const int oc = __shfl_xor(bc, off, 64);
      if (oc >= 0 && mv_before(of, oc, bf, bc)) {
        bf = of;
        bc = oc;
      }
    }
    if (lane == 0) {
      wave_f[wave] = bf;
      wave_c[wave] = bc;
    }
    __syncthreads();                                               // every y and score of the round has been read, too
    if (rd == 0 && tid == 0) top5[6] = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
    bf = wave_f[0];
    bc = wave_c[0];
#pragma unroll
    for (int w = 1; w < PFO_EVAL_THREADS / 64; ++w) {
      const double of = wave_f[w];
      const int oc = wave_c[w];
      if (oc >= 0 && mv_before(of, oc, bf, bc)) {
        bf = of;
        bc = oc;
      }
    }
    if (bc < 0) break;                                             // nobody took part (the same for every thread): the list ends
    if (tid == 0) {
      top5[rd] = bc;
      f5[rd] = bf;
      if (bc == 0 && pos_adm) top5[5] = rd;
    }
    if (tid == (bc & (PFO_EVAL_THREADS - 1))) mu[bc] = nan;        // only the picked POSITION leaves the pool
    if (rd + 1 < rounds) {
      ++n_hold;
      hold(cb[bc] - upper_u - 1);                                  // (in range: the pick was in the pool)
    }
  }
  __syncthreads();                                                 // the slots are written

  // ---- B: wavefront 0 takes the slots as its top-5
  const int plen = min(port_len[b], port_stride);
  if (tid < 64) {
    int top[5], item[5];
#pragma unroll
    for (int t = 0; t < 5; ++t) {
      top[t] = top5[t];
      item[t] = top[t] >= 0 ? cb[top[t]] : -1;
    }
    const int64_t o = out_row0 + b;
    eval_write_ranking(lane, o, top5[5], top, item, rank_out, hits, ndcg, top5_pos, top5_item);
    if (lane < 5 && m.top5_fused) m.top5_fused[o * 5 + lane] = f5[lane];
    if (lane == 0 && m.n_adm) m.n_adm[o] = top5[6];
    eval_daily_sums(daily, lane, b, plen, top, item, day_idx, port_idx, port_stride, ret_past, ret_future, n_days, n_stocks, n_ret,
                    upper_u);
  }
  eval_return_sharpe(daily, res, plen, n_ret, invest, out_row0, b);
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

extern "C" int pfo_eval_metrics_mv(const float* emb, int64_t B, int32_t D, int32_t n_neg, const int32_t* cand,
                                   const int32_t* day_idx, const int32_t* port_idx, const int32_t* port_len,
                                   int32_t port_stride, const double* ret_past, const double* ret_future, int32_t n_days,
                                   int32_t n_stocks, int32_t n_ret, int32_t upper_u, int64_t out_row0, int64_t out_rows,
                                   int32_t* rank_out, float* hits_out, float* ndcg_out, int32_t* top5_pos, int32_t* top5_item,
                                   double* invest_out, const double* ret_mv, int32_t mv_days, int32_t mv_stocks, int32_t mv_ret,
                                   const int32_t* mv_day_idx, double gamma, double lambda_mv, int32_t mode, double* top5_fused,
                                   int32_t* n_adm, float* score_out, double* y_out, double* fused_out, void* stream) {
  PFO_REQUIRE(B >= 0 && D > 0 && D % 4 == 0, "D must be a positive multiple of 4");
  PFO_REQUIRE(D <= 256, "D must be at most 256");
  PFO_REQUIRE(n_neg >= 1 && n_neg < PFO_RECOMMEND_MV_MAX_ITEMS, "1 + n_neg must be in [2, PFO_RECOMMEND_MV_MAX_ITEMS]");
  PFO_REQUIRE(n_ret >= 1 && n_ret <= PFO_EVAL_MAX_RET, "n_ret must be in [1, 128]");
  PFO_REQUIRE(mv_ret >= 2 && mv_ret <= PFO_EVAL_MAX_RET, "mv_ret must be in [2, 128]");
  PFO_REQUIRE(n_days > 0 && n_stocks > 0 && port_stride >= 0 && mv_days > 0 && mv_stocks > 0, "bad table sizes");
  PFO_REQUIRE(mode == 0 || mode == 1, "mode must be 0 (the fused list) or 1 (the basket)");
  PFO_REQUIRE(out_row0 >= 0 && out_row0 + B <= out_rows, "rows [out_row0, out_row0 + B) exceed the output buffers");
  if (B == 0) return PFO_OK;
  PFO_REQUIRE(emb && cand && day_idx && port_len && ret_past && ret_future && ret_mv && mv_day_idx, "null input");
  PFO_REQUIRE(port_idx || port_stride == 0, "null port_idx");
  PFO_REQUIRE(((uintptr_t)emb & 15) == 0, "emb must be 16-byte aligned");
  const int IC = (int)pfo_align_up(1 + n_neg, 4);
  // daily[8][n_ret] | res[16] | y, fused, mu, var, sum [IC] each | wave_f[4] | f5[6] | scores[IC] | 16 ints
  const size_t shmem = (size_t)(8 * n_ret + 16 + 5 * IC + 10) * sizeof(double) + (size_t)IC * sizeof(float) + 16 * sizeof(int);
  const EvalMvArgs m = {(int)mv_days, (int)mv_stocks, (int)mv_ret, (int)mode, gamma, lambda_mv, top5_fused, n_adm, score_out, y_out,
                        fused_out};
  const dim3 grid((unsigned)B), block(PFO_EVAL_THREADS);
  hipStream_t s = (hipStream_t)stream;
#define PFO_EVAL_MV_LAUNCH(NJ)                                                                                            \
  do {                                                                                                                    \
    if (shmem > 65536) {                                           /* more than 64 KB of dynamic LDS has to be asked for */ \
      const hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void*>(&eval_metrics_mv_kernel<NJ>),               \
                                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);                  \
      if (ea != hipSuccess) {                                                                                             \
        pfo_set_error("%s: %zu bytes of LDS refused: %s", __func__, shmem, hipGetErrorString(ea));                        \
        return PFO_ERR_HIP;                                                                                               \
      }                                                                                                                   \
    }                                                                                                                     \
    PFO_KLAUNCH(eval_metrics_mv_kernel<NJ>, grid, block, shmem, s, emb, B, (int)D, (int)n_neg, cand, day_idx, port_idx, port_len, \
                (int)port_stride, ret_past, ret_future, (int)n_days, (int)n_stocks, (int)n_ret, (int)upper_u, out_row0, rank_out, \
                hits_out, ndcg_out, top5_pos, top5_item, invest_out, ret_mv, mv_day_idx, m);                              \
  } while (0)
  switch ((D + 63) / 64) {
    case 1: PFO_EVAL_MV_LAUNCH(1); break;
    case 2: PFO_EVAL_MV_LAUNCH(2); break;
    case 3: PFO_EVAL_MV_LAUNCH(3); break;
    default: PFO_EVAL_MV_LAUNCH(4); break;
  }
#undef PFO_EVAL_MV_LAUNCH
  PFO_LAUNCH_CHECK();
  return PFO_OK;
}
