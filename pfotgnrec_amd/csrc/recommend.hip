// Read-only top-k recommendation in one launch: the scores of a tile of users against one shared candidate matrix and the k
// best admissible candidates per user, in the canonical order of SURVEY App. A-9 (score descending, the LARGER position first
// among equal scores - the order pfo_eval_metrics ranks in).  The U x I score matrix never reaches HBM.
//
// One workgroup of four wavefronts per 16 users.
//   A  scores.  v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation): users are the rows, 16 candidates the columns.
//      A dot product does not care in which order its terms are taken, so k-slot q of the c-th of four MFMAs stands for element
//      16 j + 4 q + c of both rows: lane (r, q) then reads its operand as ONE 16-byte load at floats [16 j + 4 q, + 4) of row r,
//      four lanes cover 64 contiguous bytes of a row.  The user fragments stay in registers for the whole kernel; wavefront w takes
//      the candidate tiles w, w + 4, ...  Scores go to LDS as [16 users][chunk], at most PFO_REC_CHUNK candidates at a time.
//   B  selection.  A wavefront owns four users and runs their rounds interleaved (four independent reduction chains).  A
//      candidate is the 64-bit key (score mapped to an order-preserving unsigned | position): the canonical order is the plain
//      unsigned order of the keys, 0 = nothing.  Lane l keeps the keys of candidates l, l + 64, ... of the chunk in registers
//      (inadmissible ones as 0) and ONE key of the list found so far - lane t holds rank t (k <= 64).  A round is a wave-wide
//      maximum over both; the owner of the winner clears it.  After k rounds the winners are the new list, so a candidate
//      list longer than a chunk is a walk over chunks with the list carried along.
// Users of one tile that sit in different blocks are served block by block (a pass per distinct block of the tile; callers
// that sort their users by block get one pass).
#include "common.hpp"
#include "mv_value.hpp"

#define PFO_REC_THREADS 256
#define PFO_REC_TILE 16                       // users per workgroup = rows of the MFMA tile
#define PFO_REC_CHUNK 512                     // candidates whose scores are in LDS at a time (32 KB)
#define PFO_REC_SLOTS (PFO_REC_CHUNK / 64)    // keys per lane and user

namespace {

typedef float rec_f32x4 __attribute__((ext_vector_type(4)));

// fp32 -> unsigned with the same order; -0 and +0 share a key (they are equal scores)
__device__ __forceinline__ uint32_t rec_ordered(float s) {
  uint32_t b = __float_as_uint(s);
  if (b == 0x80000000u) b = 0u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float rec_unordered(uint32_t o) {
  return __uint_as_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o);
}
__device__ __forceinline__ unsigned long long rec_max(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

// One 16 x 16 tile of scores: acc[i] = user row 4 q + i . candidate row `item` (this lane's column), uf the lane's pieces of its
// user row.  The ONE place the accumulation order of a score is written down: both kernels below call it, so they agree to the bit.
template <int NJ>
__device__ __forceinline__ rec_f32x4 rec_score_tile(const float4 (&uf)[NJ], const float* __restrict__ items, int item, int D, int q) {
  const float4* ip = reinterpret_cast<const float4*>(items + (int64_t)item * D);
  float4 v[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int d = 16 * j + 4 * q;
    v[j] = d < D ? ip[d >> 2] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  rec_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(uf[j].x, v[j].x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(uf[j].y, v[j].y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(uf[j].z, v[j].z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(uf[j].w, v[j].w, acc, 0, 0, 0);
  }
  return acc;
}

// NJ 16-byte pieces per lane cover a row of D <= 16 * NJ floats
template <int NJ>
__global__ __launch_bounds__(PFO_REC_THREADS) void recommend_topk_kernel(
    const float* __restrict__ user_emb, const float* __restrict__ item_emb, const int32_t* __restrict__ user_block, int64_t U,
    int I, int n_t, int D, const int32_t* __restrict__ excl_pos, const int32_t* __restrict__ excl_len, int excl_stride,
    const uint8_t* __restrict__ item_ok, int k, int32_t* __restrict__ top_pos, float* __restrict__ top_score,
    int32_t* __restrict__ n_valid, int IC) {
  const int ICS = IC + 4;                                            // row stride: the four user rows a half-wave writes fall on different banks
  extern __shared__ float lds[];
  float* sc = lds;                                                    // [16][ICS]
  uint8_t* ok = reinterpret_cast<uint8_t*>(sc + PFO_REC_TILE * ICS);  // [IC]
  __shared__ int ub[PFO_REC_TILE];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, q = lane >> 4;
  const int64_t u0 = (int64_t)blockIdx.x * PFO_REC_TILE;

  if (tid < PFO_REC_TILE) {
    const int64_t u = u0 + tid;
    int b = -1;                                                      // a row beyond U: served by no pass
    if (u < U) b = user_block ? min(max(user_block[u], 0), n_t - 1) : 0;
    ub[tid] = b;
  }
  // this lane's pieces of user row r (a row beyond U reads the last user's: its scores are never selected from)
  float4 uf[NJ];
  {
    const float4* up = reinterpret_cast<const float4*>(user_emb + min(u0 + r, U - 1) * D);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int d = 16 * j + 4 * q;
      uf[j] = d < D ? up[d >> 2] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  __syncthreads();
  unsigned pending = 0;
#pragma unroll
  for (int i = 0; i < PFO_REC_TILE; ++i) pending |= (ub[i] >= 0 ? 1u : 0u) << i;

  while (pending) {                                                  // one pass per distinct block of the tile
    const int b = ub[__ffs(pending) - 1];
    unsigned members = 0;
#pragma unroll
    for (int i = 0; i < PFO_REC_TILE; ++i) members |= (((pending >> i) & 1u) && ub[i] == b ? 1u : 0u) << i;
    pending &= ~members;
    const float* items = item_emb + (int64_t)b * I * D;

    unsigned long long list[4] = {0ull, 0ull, 0ull, 0ull};           // lane t: rank t of user 4 * wave + i so far
    for (int c0 = 0; c0 < I; c0 += IC) {
      const int n = min(IC, I - c0);
      __syncthreads();                                               // the previous chunk's keys have been taken from LDS
      // ---- A: scores of candidates [c0, c0 + n)
      const int n_tile = (n + 15) >> 4;
      for (int t = wave; t < n_tile; t += 4) {
        const rec_f32x4 acc = rec_score_tile<NJ>(uf, items, min(c0 + 16 * t + r, I - 1), D, q);   // (a column beyond I repeats the last row; never read back)
        // acc[i] = score(user 4 q + i, candidate 16 t + r)
#pragma unroll
        for (int i = 0; i < 4; ++i) sc[(4 * q + i) * ICS + 16 * t + r] = acc[i];
      }
      for (int c = tid; c < n; c += PFO_REC_THREADS) ok[c] = item_ok ? item_ok[c0 + c] : (uint8_t)1;
      __syncthreads();

      // ---- B: this wavefront's four users
      unsigned long long key[4][PFO_REC_SLOTS];
      bool any_member = false;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int us = 4 * wave + i;
        const bool member = (members >> us) & 1u;
        any_member |= member;
        unsigned adm = 0;                                            // bit m: candidate lane + 64 m of the chunk is admissible
        if (member) {
#pragma unroll
          for (int m = 0; m < PFO_REC_SLOTS; ++m) {
            const int c = lane + 64 * m;
            if (c < n && ok[c]) adm |= 1u << m;
          }
          const int64_t u = u0 + us;
          const int len = (excl_pos && excl_stride > 0) ? min(max(excl_len[u], 0), excl_stride) : 0;
          for (int e0 = 0; e0 < len; e0 += 64) {
            int rel = -1;                                            // position within the chunk, -1: not in it
            if (e0 + lane < len) {
              const int p = excl_pos[u * excl_stride + e0 + lane];
              if (p >= c0 && p < c0 + n) rel = p - c0;
            }
            const int cnt = min(64, len - e0);
            for (int j = 0; j < cnt; ++j) {
              const int rj = __builtin_amdgcn_readlane(rel, j);
              if (rj >= 0 && (rj & 63) == lane) adm &= ~(1u << (rj >> 6));
            }
          }
        }
#pragma unroll
        for (int m = 0; m < PFO_REC_SLOTS; ++m) {
          const int c = lane + 64 * m;
          unsigned long long kk = 0ull;
          if ((adm >> m) & 1u) kk = ((unsigned long long)rec_ordered(sc[us * ICS + c]) << 32) | (unsigned)(c0 + c);
          key[i][m] = kk;
        }
      }
      if (any_member) {
        unsigned long long next[4] = {0ull, 0ull, 0ull, 0ull};
        for (int t = 0; t < k; ++t) {
          unsigned long long best[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            best[i] = list[i];
#pragma unroll
            for (int m = 0; m < PFO_REC_SLOTS; ++m) best[i] = rec_max(best[i], key[i][m]);
          }
#pragma unroll
          for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
            for (int i = 0; i < 4; ++i) best[i] = rec_max(best[i], __shfl_xor(best[i], off, 64));
          }
          if ((best[0] | best[1] | best[2] | best[3]) == 0ull) break;     // nothing admissible is left for any of the four
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            if (best[i] == 0ull) continue;
            // positions are distinct, so exactly one key of the wavefront equals the winner: its owner clears it
            if (list[i] == best[i]) list[i] = 0ull;
#pragma unroll
            for (int m = 0; m < PFO_REC_SLOTS; ++m)
              if (key[i][m] == best[i]) key[i][m] = 0ull;
            if (lane == t) next[i] = best[i];
          }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) list[i] = next[i];
      }
    }

    // ---- the list of every user of this pass
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int us = 4 * wave + i;
      if (!((members >> us) & 1u)) continue;
      const int64_t u = u0 + us;
      const bool got = lane < k && list[i] != 0ull;
      if (lane < k) {
        top_pos[u * k + lane] = got ? (int32_t)(uint32_t)(list[i] & 0xffffffffull) : -1;
        top_score[u * k + lane] = got ? rec_unordered((uint32_t)(list[i] >> 32)) : -__builtin_inff();
      }
      const int cnt = __popcll(__ballot(got));
      if (lane == 0 && n_valid) n_valid[u] = cnt;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Portfolio-aware top-k: the rank fusion of main.py:243-289 over the WHOLE candidate list of a user, in the same launch shape.
//   A  scores of the tile's 16 users against ALL I <= 2048 candidates of a block, as above (rec_score_tile), into LDS [16][I].
//   Then the users of the pass one at a time, all four wavefronts on one user:
//   B  y_mv of every candidate in fp64 (pfo_mv_value, the arithmetic mv_select_kernel runs) into LDS y[I]; a candidate that is
//      not admissible - item_ok, cand_stock or the day outside the tables, a NaN y, then the exclusion list - is a NaN there:
//      every comparison with it is false, so it takes part in no count below.
//   C  average-tie ranks of y and of the fp32 score by counting over LDS (scipy's rankdata is less + (equal + 1) / 2), blended
//      into `fused` in registers (a thread owns candidates tid, tid + 256, ...: eight at most); after a barrier fused replaces y.
//   D  the place of a candidate in the canonical order (fused descending, the larger position first among equal values) is
//      the number of candidates before it, by counting again; places below k write the output row.
// LDS: 8 I (y / fused) + 16 (I + 4) 4 (scores) bytes, 144 KB at I = 2048 of the 160 KB a workgroup may take - one workgroup per
// CU there, four at I = 500.  About 3 I^2 comparisons per user.
#define PFO_RMV_PER_THREAD (PFO_RECOMMEND_MV_MAX_ITEMS / PFO_REC_THREADS)

template <int NJ>
__global__ __launch_bounds__(PFO_REC_THREADS) void recommend_mv_topk_kernel(
    const float* __restrict__ user_emb, const float* __restrict__ item_emb, const int32_t* __restrict__ user_block, int64_t U,
    int I, int n_t, int D, const int32_t* __restrict__ excl_pos, const int32_t* __restrict__ excl_len, int excl_stride,
    const uint8_t* __restrict__ item_ok, const int32_t* __restrict__ cand_stock, const double* __restrict__ returns, int n_days,
    int n_stocks, int n_ret, const int32_t* __restrict__ day_idx, const int32_t* __restrict__ port_idx,
    const int32_t* __restrict__ port_len, int port_stride, double gamma, double lam, int k, int32_t* __restrict__ top_pos,
    float* __restrict__ top_score, double* __restrict__ top_fused, int32_t* __restrict__ n_valid, float* __restrict__ score_out,
    double* __restrict__ y_out, double* __restrict__ fused_out, int IC) {
  const int ICS = IC + 4;
  extern __shared__ double lds_mv[];
  double* yv = lds_mv;                                               // [IC]: y, then fused, of the user being ranked
  float* sc = reinterpret_cast<float*>(yv + IC);                     // [16][ICS]
  __shared__ int ub[PFO_REC_TILE];
  __shared__ int n_adm;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, q = lane >> 4;
  const int64_t u0 = (int64_t)blockIdx.x * PFO_REC_TILE;
  const double nan = __builtin_nan("");

  if (tid < PFO_REC_TILE) {
    const int64_t u = u0 + tid;
    int b = -1;
    if (u < U) b = user_block ? min(max(user_block[u], 0), n_t - 1) : 0;
    ub[tid] = b;
  }
  float4 uf[NJ];
  {
    const float4* up = reinterpret_cast<const float4*>(user_emb + min(u0 + r, U - 1) * D);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int d = 16 * j + 4 * q;
      uf[j] = d < D ? up[d >> 2] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  __syncthreads();
  unsigned pending = 0;
#pragma unroll
  for (int i = 0; i < PFO_REC_TILE; ++i) pending |= (ub[i] >= 0 ? 1u : 0u) << i;

  while (pending) {                                                  // one pass per distinct block of the tile
    const int b = ub[__ffs(pending) - 1];
    unsigned members = 0;
#pragma unroll
    for (int i = 0; i < PFO_REC_TILE; ++i) members |= (((pending >> i) & 1u) && ub[i] == b ? 1u : 0u) << i;
    pending &= ~members;
    const float* items = item_emb + (int64_t)b * I * D;

    // ---- A: scores of all candidates (the previous pass ended on a barrier)
    const int n_tile = (I + 15) >> 4;
    for (int t = wave; t < n_tile; t += 4) {
      const rec_f32x4 acc = rec_score_tile<NJ>(uf, items, min(16 * t + r, I - 1), D, q);
#pragma unroll
      for (int i = 0; i < 4; ++i) sc[(4 * q + i) * ICS + 16 * t + r] = acc[i];
    }
    __syncthreads();

    for (int us = 0; us < PFO_REC_TILE; ++us) {
      if (!((members >> us) & 1u)) continue;                         // (the same for every thread)
      const int64_t u = u0 + us;
      const float* su = sc + us * ICS;
      if (tid == 0) n_adm = 0;
      // ---- B: y_mv, NaN where the candidate is not admissible
      const int day = day_idx[u];
      const bool day_ok = day >= 0 && day < n_days;                  // no day: nothing of this user's is read
      const int plen = (day_ok && port_idx && port_stride > 0) ? min(max(port_len[u], 0), port_stride) : 0;
      const double* dayp = returns + (int64_t)(day_ok ? day : 0) * n_stocks * n_ret;
      for (int c = tid; c < I; c += PFO_REC_THREADS) {
        if (score_out) score_out[u * I + c] = su[c];
        double y = nan;
        if (day_ok && (!item_ok || item_ok[c])) {
          const int stock = cand_stock[c];
          if (stock >= 0 && stock < n_stocks)
            y = pfo_mv_value<true>(dayp, stock, n_stocks, n_ret, port_idx + u * port_stride, plen, gamma);
        }
        yv[c] = y;
      }
      __syncthreads();
      {
        const int len = (excl_pos && excl_stride > 0) ? min(max(excl_len[u], 0), excl_stride) : 0;
        for (int e = tid; e < len; e += PFO_REC_THREADS) {
          const int p = excl_pos[u * excl_stride + e];
          if (p >= 0 && p < I) yv[p] = nan;                          // (duplicates store the same value)
        }
      }
      __syncthreads();
      // ---- C: ranks over the admissible candidates, blended
      double fused[PFO_RMV_PER_THREAD];
      int mine = 0;
#pragma unroll
      for (int m = 0; m < PFO_RMV_PER_THREAD; ++m) fused[m] = nan;
#pragma unroll
      for (int m = 0; m < PFO_RMV_PER_THREAD; ++m) {
        const int c = tid + PFO_REC_THREADS * m;
        if (PFO_REC_THREADS * m >= I) break;
        if (c >= I) continue;
        const double yi = yv[c];
        if (y_out) y_out[u * I + c] = yi;
        if (!(yi == yi)) continue;
        const float si = su[c];
        int ly = 0, ey = 0, ls = 0, es = 0;
        for (int j = 0; j < I; ++j) {
          const double yj = yv[j];
          const float sj = su[j];
          const bool aj = yj == yj;
          ly += (yj < yi);
          ey += (yj == yi);
          ls += (aj && sj < si);
          es += (aj && sj == si);                                    // (-0 == +0)
        }
        fused[m] = pfo_mv_blend(pfo_mv_avg_rank(ly, ey), pfo_mv_avg_rank(ls, es), lam);   // main.py:282-286
        ++mine;
      }
      __syncthreads();                                               // every y has been read
#pragma unroll
      for (int m = 0; m < PFO_RMV_PER_THREAD; ++m) {
        const int c = tid + PFO_REC_THREADS * m;
        if (c < I) {
          yv[c] = fused[m];
          if (fused_out) fused_out[u * I + c] = fused[m];
        }
      }
      if (mine) atomicAdd(&n_adm, mine);
      __syncthreads();
      // ---- D: the first k of the canonical order
#pragma unroll
      for (int m = 0; m < PFO_RMV_PER_THREAD; ++m) {
        const int c = tid + PFO_REC_THREADS * m;
        if (PFO_REC_THREADS * m >= I) break;
        const double fi = fused[m];
        if (c >= I || !(fi == fi)) continue;
        int before = 0;
        for (int j = 0; j < I; ++j) {
          const double fj = yv[j];
          before += (fj > fi) || (fj == fi && j > c);
        }
        if (before < k) {
          const float s = su[c];
          top_pos[u * k + before] = c;
          top_score[u * k + before] = s == 0.f ? 0.f : s;            // a zero score is handed out as +0
          top_fused[u * k + before] = fi;
        }
      }
      const int n = min(k, n_adm);
      if (tid >= n && tid < k) {
        top_pos[u * k + tid] = -1;
        top_score[u * k + tid] = -__builtin_inff();
        top_fused[u * k + tid] = -__builtin_inf();
      }
      if (tid == 0 && n_valid) n_valid[u] = n;
      __syncthreads();                                               // n_adm and y are free for the next user
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Basket top-k: the list of recommend_mv_topk_kernel taken one pick at a time, each pick joining the holdings before the next
// is ranked (include/pfotgn.h states the rounds).  Same launch shape and the same stage A.  Per user, all four wavefronts:
//   B  the admissible set once - item_ok, cand_stock and the day, then the exclusion list scattered over LDS y[I] - read back
//      into a bit per owned candidate (a thread owns candidates tid, tid + 256, ...); mu, var and the covariance sum over the
//      portfolio of every owned candidate in registers (pfo_mv_mean / pfo_mv_var / pfo_mv_add_cov: pfo_mv_value's pieces).
//   k rounds of
//   C  y of the round from the three registers (pfo_mv_finish) into LDS y[I], NaN where the candidate takes no part, and NaN
//      over its score in the user's LDS row likewise (the owner keeps the score in a register; the row is this user's alone):
//      the two rank counts of stage C above then need no mask, and run over four candidates per LDS read (y and the row are
//      NaN from I up to the next multiple of 16); the blend as above;
//   P  the pick: the arg-max of (fused, position) over the thread's candidates, the wavefront (shuffles), the workgroup (four
//      LDS slots).  Its owner writes slot r of the output row, clears its bit and sets y[pick] to NaN; every thread adds the
//      pick's covariance to its candidates' sums - one n_ret-long pass per candidate and round, nothing else is recomputed.
// LDS as above (the per-candidate values are registers; the dynamic part starts 16-byte aligned for the wide reads).
// 2 k I^2 comparisons and (held + k - 1) I n_ret multiply-adds per user.
// Two barriers per round; every loop bound between them depends on k, I and the pick (the same for all threads) alone.
template <int NJ>
__global__ __launch_bounds__(PFO_REC_THREADS) void recommend_basket_topk_kernel(
    const float* __restrict__ user_emb, const float* __restrict__ item_emb, const int32_t* __restrict__ user_block, int64_t U,
    int I, int n_t, int D, const int32_t* __restrict__ excl_pos, const int32_t* __restrict__ excl_len, int excl_stride,
    const uint8_t* __restrict__ item_ok, const int32_t* __restrict__ cand_stock, const double* __restrict__ returns, int n_days,
    int n_stocks, int n_ret, const int32_t* __restrict__ day_idx, const int32_t* __restrict__ port_idx,
    const int32_t* __restrict__ port_len, int port_stride, double gamma, double lam, int k, int32_t* __restrict__ top_pos,
    float* __restrict__ top_score, double* __restrict__ top_fused, int32_t* __restrict__ n_valid, int IC) {
  const int ICS = IC + 4;
  extern __shared__ __attribute__((aligned(16))) double lds_basket[];
  double* yv = lds_basket;                                           // [IC]: y of the round, NaN = takes no part
  float* sc = reinterpret_cast<float*>(yv + IC);                     // [16][ICS]
  __shared__ int ub[PFO_REC_TILE];
  __shared__ double wave_f[PFO_REC_THREADS / 64];                    // the best (fused, position) of each wavefront
  __shared__ int wave_c[PFO_REC_THREADS / 64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, q = lane >> 4;
  const int64_t u0 = (int64_t)blockIdx.x * PFO_REC_TILE;
  const double nan = __builtin_nan("");
  const double inv = pfo_mv_inv(n_ret);

  if (tid < PFO_REC_TILE) {
    const int64_t u = u0 + tid;
    int b = -1;
    if (u < U) b = user_block ? min(max(user_block[u], 0), n_t - 1) : 0;
    ub[tid] = b;
  }
  float4 uf[NJ];
  {
    const float4* up = reinterpret_cast<const float4*>(user_emb + min(u0 + r, U - 1) * D);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int d = 16 * j + 4 * q;
      uf[j] = d < D ? up[d >> 2] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  __syncthreads();
  unsigned pending = 0;
#pragma unroll
  for (int i = 0; i < PFO_REC_TILE; ++i) pending |= (ub[i] >= 0 ? 1u : 0u) << i;

  while (pending) {                                                  // one pass per distinct block of the tile
    const int b = ub[__ffs(pending) - 1];
    unsigned members = 0;
#pragma unroll
    for (int i = 0; i < PFO_REC_TILE; ++i) members |= (((pending >> i) & 1u) && ub[i] == b ? 1u : 0u) << i;
    pending &= ~members;
    const float* items = item_emb + (int64_t)b * I * D;

    // ---- A: scores of all candidates (the previous pass ended on a barrier)
    const int n_tile = (I + 15) >> 4;
    for (int t = wave; t < n_tile; t += 4) {
      const rec_f32x4 acc = rec_score_tile<NJ>(uf, items, min(16 * t + r, I - 1), D, q);
#pragma unroll
      for (int i = 0; i < 4; ++i) sc[(4 * q + i) * ICS + 16 * t + r] = acc[i];
    }
    __syncthreads();

    for (int us = 0; us < PFO_REC_TILE; ++us) {
      if (!((members >> us) & 1u)) continue;                         // (the same for every thread)
      const int64_t u = u0 + us;
      float* su = sc + us * ICS;                                     // the user's scores; NaN where the candidate takes no part
      const int day = day_idx[u];
      const bool day_ok = day >= 0 && day < n_days;                  // no day: nothing of this user's is read
      const int plen = (day_ok && port_idx && port_stride > 0) ? min(max(port_len[u], 0), port_stride) : 0;
      const double* dayp = returns + (int64_t)(day_ok ? day : 0) * n_stocks * n_ret;
      // ---- B: the admissible set, then mu, var and the covariance sum over the portfolio
      for (int c = tid; c < I; c += PFO_REC_THREADS) {
        bool ok = day_ok && (!item_ok || item_ok[c]);
        if (ok) {
          const int stock = cand_stock[c];
          ok = stock >= 0 && stock < n_stocks;
        }
        yv[c] = ok ? 0.0 : nan;
      }
      for (int c = I + tid; c < IC; c += PFO_REC_THREADS) yv[c] = nan;
      __syncthreads();
      {
        const int len = (excl_pos && excl_stride > 0) ? min(max(excl_len[u], 0), excl_stride) : 0;
        for (int e = tid; e < len; e += PFO_REC_THREADS) {
          const int p = excl_pos[u * excl_stride + e];
          if (p >= 0 && p < I) yv[p] = nan;                          // (duplicates store the same value)
        }
      }
      __syncthreads();
      double mu[PFO_RMV_PER_THREAD], var[PFO_RMV_PER_THREAD], ssum[PFO_RMV_PER_THREAD];
      float score[PFO_RMV_PER_THREAD];
      unsigned alive = 0;                                            // bit m: candidate tid + 256 m is in the pool
#pragma unroll
      for (int m = 0; m < PFO_RMV_PER_THREAD; ++m) {
        const int c = tid + PFO_REC_THREADS * m;
        mu[m] = var[m] = ssum[m] = 0.0;
        score[m] = 0.f;
        if (c < I && yv[c] == yv[c]) {
          alive |= 1u << m;
          score[m] = su[c];
          const double* ri = dayp + (int64_t)cand_stock[c] * n_ret;
          mu[m] = pfo_mv_mean(ri, n_ret);
          var[m] = pfo_mv_var(ri, mu[m], n_ret, inv);
        } else if (c < IC) {
          su[c] = __builtin_nanf("");
        }
      }
      // one more holding: row s of the day (in range) joins every pooled candidate's sum
      auto hold = [&](int s) {
        const double* rp = dayp + (int64_t)s * n_ret;
        const double mp = pfo_mv_mean(rp, n_ret);
#pragma unroll
        for (int m = 0; m < PFO_RMV_PER_THREAD; ++m) {
          if (!((alive >> m) & 1u)) continue;
          const double* ri = dayp + (int64_t)cand_stock[tid + PFO_REC_THREADS * m] * n_ret;
          ssum[m] = pfo_mv_add_cov(ssum[m], ri, mu[m], rp, mp, n_ret, inv);
        }
      };
      int n_hold = 0;
      for (int p = 0; p < plen; ++p) {
        const int s = port_idx[u * port_stride + p];
        if ((unsigned)s >= (unsigned)n_stocks) continue;
        ++n_hold;
        hold(s);
      }

      int n_pick = 0;
      for (int rd = 0; rd < k; ++rd) {
        // ---- C: y of this round (the slot of a candidate outside the pool is NaN already), ranks, blend
        double yr[PFO_RMV_PER_THREAD];
#pragma unroll
        for (int m = 0; m < PFO_RMV_PER_THREAD; ++m) {
          yr[m] = nan;
          if (!((alive >> m) & 1u)) continue;
          const int c = tid + PFO_REC_THREADS * m;
          yr[m] = pfo_mv_finish(mu[m], gamma, var[m], ssum[m], n_hold);
          yv[c] = yr[m];
          su[c] = yr[m] == yr[m] ? score[m] : __builtin_nanf("");
        }
        __syncthreads();
        double bf = 0.0;
        int bc = -1;                                                 // the best (fused, position) so far, -1: none
#pragma unroll
        for (int m = 0; m < PFO_RMV_PER_THREAD; ++m) {
          const int c = tid + PFO_REC_THREADS * m;
          const double yi = yr[m];
          if (!(yi == yi)) continue;                                 // outside the pool, or a NaN y: out of this round only
          const float si = score[m];
          int ly = 0, ey = 0, ls = 0, es = 0;
          const double2* y2 = reinterpret_cast<const double2*>(yv);
          const float4* s4 = reinterpret_cast<const float4*>(su);
#pragma unroll 2
          for (int j = 0; j < IC; j += 4) {                          // (every comparison with a NaN is false)
            const double2 ya = y2[j >> 1], yb = y2[(j >> 1) + 1];
            const float4 sj = s4[j >> 2];
            ly += (ya.x < yi) + (ya.y < yi) + (yb.x < yi) + (yb.y < yi);
            ey += (ya.x == yi) + (ya.y == yi) + (yb.x == yi) + (yb.y == yi);
            ls += (sj.x < si) + (sj.y < si) + (sj.z < si) + (sj.w < si);
            es += (sj.x == si) + (sj.y == si) + (sj.z == si) + (sj.w == si);   // (-0 == +0)
          }
          const double f = pfo_mv_blend(pfo_mv_avg_rank(ly, ey), pfo_mv_avg_rank(ls, es), lam);   // main.py:282-286
          if (f == f && (bc < 0 || f > bf || (f == bf && c > bc))) {
            bf = f;
            bc = c;
          }
        }
        // ---- P: the first of the canonical order
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
          const double of = __shfl_xor(bf, off, 64);
          const int oc = __shfl_xor(bc, off, 64);
          if (oc >= 0 && (bc < 0 || of > bf || (of == bf && oc > bc))) {
            bf = of;
            bc = oc;
          }
        }
        if (lane == 0) {
          wave_f[wave] = bf;
          wave_c[wave] = bc;
        }
        __syncthreads();                                             // every y of the round has been read, too
        bf = wave_f[0];
        bc = wave_c[0];
#pragma unroll
        for (int w = 1; w < PFO_REC_THREADS / 64; ++w) {
          const double of = wave_f[w];
          const int oc = wave_c[w];
          if (oc >= 0 && (bc < 0 || of > bf || (of == bf && oc > bc))) {
            bf = of;
            bc = oc;
          }
        }
        if (bc < 0) break;                                           // nobody took part (the same for every thread): the list ends
        if (tid == (bc & (PFO_REC_THREADS - 1))) {
          alive &= ~(1u << (bc / PFO_REC_THREADS));
          yv[bc] = nan;
          const float s = su[bc];
          su[bc] = __builtin_nanf("");
          top_pos[u * k + rd] = bc;
          top_score[u * k + rd] = s == 0.f ? 0.f : s;                // a zero score is handed out as +0
          top_fused[u * k + rd] = bf;
        }
        ++n_pick;
        if (rd + 1 < k) {
          ++n_hold;
          hold(cand_stock[bc]);                                      // (in range: the pick was in the pool)
        }
      }
      for (int t = n_pick + tid; t < k; t += PFO_REC_THREADS) {
        top_pos[u * k + t] = -1;
        top_score[u * k + t] = -__builtin_inff();
        top_fused[u * k + t] = -__builtin_inf();
      }
      if (tid == 0 && n_valid) n_valid[u] = n_pick;
      __syncthreads();                                               // y and the wavefront slots are free for the next user
    }
  }
}

}  // namespace

extern "C" int pfo_recommend_topk(const float* user_emb, const float* item_emb, const int32_t* user_block, int64_t U, int32_t I,
                                  int32_t n_t, int32_t D, const int32_t* excl_pos, const int32_t* excl_len, int32_t excl_stride,
                                  const uint8_t* item_ok, int32_t k, int32_t* top_pos, float* top_score, int32_t* n_valid,
                                  void* stream) {
  PFO_REQUIRE(U >= 0 && U <= (int64_t)PFO_REC_TILE * 0x7fffffff, "U out of range");
  PFO_REQUIRE(D > 0 && D % 4 == 0, "D must be a positive multiple of 4");
  PFO_REQUIRE(D <= 256, "D must be at most 256");
  PFO_REQUIRE(k >= 1 && k <= 64, "k must be in [1, 64]");
  PFO_REQUIRE(I >= 1 && I <= PFO_RECOMMEND_MAX_ITEMS, "I must be in [1, PFO_RECOMMEND_MAX_ITEMS]");
  PFO_REQUIRE(n_t >= 1 && (int64_t)n_t * I <= 0x7fffffff, "n_t must be at least 1 and n_t * I fit 31 bits");
  PFO_REQUIRE(excl_stride >= 0, "excl_stride must not be negative");
  if (U == 0) return PFO_OK;
  PFO_REQUIRE(user_emb && item_emb && top_pos && top_score, "null input or output");
  PFO_REQUIRE(!excl_pos || excl_stride == 0 || excl_len, "excl_pos without excl_len");
  PFO_REQUIRE((((uintptr_t)user_emb | (uintptr_t)item_emb) & 15) == 0, "user_emb and item_emb must be 16-byte aligned");
  const int IC = (int)pfo_align_up(I < PFO_REC_CHUNK ? I : PFO_REC_CHUNK, 16);
  const size_t shmem = (size_t)PFO_REC_TILE * (IC + 4) * sizeof(float) + (size_t)IC;
  const dim3 grid((unsigned)pfo_ceil_div(U, PFO_REC_TILE)), block(PFO_REC_THREADS);
  hipStream_t s = (hipStream_t)stream;
#define PFO_REC_LAUNCH(NJ)                                                                                              \
  PFO_KLAUNCH(recommend_topk_kernel<NJ>, grid, block, shmem, s, user_emb, item_emb, user_block, U, (int)I, (int)n_t, (int)D, \
              excl_pos, excl_len, (int)excl_stride, item_ok, (int)k, top_pos, top_score, n_valid, IC)
  const int nj = (D + 15) / 16;
  if (nj <= 2) PFO_REC_LAUNCH(2);
  else if (nj <= 4) PFO_REC_LAUNCH(4);
  else if (nj <= 8) PFO_REC_LAUNCH(8);
  else if (nj <= 11) PFO_REC_LAUNCH(11);
  else PFO_REC_LAUNCH(16);
#undef PFO_REC_LAUNCH
  PFO_LAUNCH_CHECK();
  return PFO_OK;
}

extern "C" int pfo_recommend_mv_topk(const float* user_emb, const float* item_emb, const int32_t* user_block, int64_t U, int32_t I,
                                     int32_t n_t, int32_t D, const int32_t* excl_pos, const int32_t* excl_len, int32_t excl_stride,
                                     const uint8_t* item_ok, const int32_t* cand_stock, const double* returns, int32_t n_days,
                                     int32_t n_stocks, int32_t n_ret, const int32_t* day_idx, const int32_t* port_idx,
                                     const int32_t* port_len, int32_t port_stride, double gamma, double lambda_mv, int32_t k,
                                     int32_t* top_pos, float* top_score, double* top_fused, int32_t* n_valid, float* score_out,
                                     double* y_out, double* fused_out, void* stream) {
  PFO_REQUIRE(U >= 0 && U <= (int64_t)PFO_REC_TILE * 0x7fffffff, "U out of range");
  PFO_REQUIRE(D > 0 && D % 4 == 0, "D must be a positive multiple of 4");
  PFO_REQUIRE(D <= 256, "D must be at most 256");
  PFO_REQUIRE(k >= 1 && k <= 64, "k must be in [1, 64]");
  PFO_REQUIRE(I >= 1 && I <= PFO_RECOMMEND_MV_MAX_ITEMS, "I must be in [1, PFO_RECOMMEND_MV_MAX_ITEMS]");
  PFO_REQUIRE(n_t >= 1 && (int64_t)n_t * I <= 0x7fffffff, "n_t must be at least 1 and n_t * I fit 31 bits");
  PFO_REQUIRE(excl_stride >= 0 && port_stride >= 0, "excl_stride and port_stride must not be negative");
  PFO_REQUIRE(n_ret >= 2 && n_ret <= 128, "n_ret must be in [2, 128]");
  PFO_REQUIRE(n_days > 0 && n_stocks > 0, "n_days and n_stocks must be positive");
  if (U == 0) return PFO_OK;
  PFO_REQUIRE(user_emb && item_emb && top_pos && top_score && top_fused, "null input or output");
  PFO_REQUIRE(cand_stock && returns && day_idx, "null mean-variance input");
  PFO_REQUIRE(!excl_pos || excl_stride == 0 || excl_len, "excl_pos without excl_len");
  PFO_REQUIRE(!port_idx || port_stride == 0 || port_len, "port_idx without port_len");
  PFO_REQUIRE((((uintptr_t)user_emb | (uintptr_t)item_emb) & 15) == 0, "user_emb and item_emb must be 16-byte aligned");
  const int IC = (int)pfo_align_up(I, 16);
  const size_t shmem = (size_t)IC * sizeof(double) + (size_t)PFO_REC_TILE * (IC + 4) * sizeof(float);
  const dim3 grid((unsigned)pfo_ceil_div(U, PFO_REC_TILE)), block(PFO_REC_THREADS);
  hipStream_t s = (hipStream_t)stream;
  // (more than 64 KB of dynamic LDS has to be asked for, per kernel)
#define PFO_RMV_LAUNCH(NJ)                                                                                                   \
  do {                                                                                                                       \
    if (shmem > 65536) {                                                                                                     \
      const hipError_t ea__ = hipFuncSetAttribute(reinterpret_cast<const void*>(&recommend_mv_topk_kernel<NJ>),              \
                                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);                   \
      if (ea__ != hipSuccess) {                                                                                              \
        pfo_set_error("%s: %zu bytes of LDS refused: %s", __func__, shmem, hipGetErrorString(ea__));                         \
        return PFO_ERR_HIP;                                                                                                  \
      }                                                                                                                      \
    }                                                                                                                        \
    PFO_KLAUNCH(recommend_mv_topk_kernel<NJ>, grid, block, shmem, s, user_emb, item_emb, user_block, U, (int)I, (int)n_t,    \
                (int)D, excl_pos, excl_len, (int)excl_stride, item_ok, cand_stock, returns, (int)n_days, (int)n_stocks,      \
                (int)n_ret, day_idx, port_idx, port_len, (int)port_stride, gamma, lambda_mv, (int)k, top_pos, top_score,     \
                top_fused, n_valid, score_out, y_out, fused_out, IC);                                                        \
  } while (0)
  const int nj = (D + 15) / 16;
  if (nj <= 2) PFO_RMV_LAUNCH(2);
  else if (nj <= 4) PFO_RMV_LAUNCH(4);
  else if (nj <= 8) PFO_RMV_LAUNCH(8);
  else if (nj <= 11) PFO_RMV_LAUNCH(11);
  else PFO_RMV_LAUNCH(16);
#undef PFO_RMV_LAUNCH
  PFO_LAUNCH_CHECK();
  return PFO_OK;
}

extern "C" int pfo_recommend_basket_topk(const float* user_emb, const float* item_emb, const int32_t* user_block, int64_t U,
                                         int32_t I, int32_t n_t, int32_t D, const int32_t* excl_pos, const int32_t* excl_len,
                                         int32_t excl_stride, const uint8_t* item_ok, const int32_t* cand_stock,
                                         const double* returns, int32_t n_days, int32_t n_stocks, int32_t n_ret,
                                         const int32_t* day_idx, const int32_t* port_idx, const int32_t* port_len,
                                         int32_t port_stride, double gamma, double lambda_mv, int32_t k, int32_t* top_pos,
                                         float* top_score, double* top_fused, int32_t* n_valid, void* stream) {
  PFO_REQUIRE(U >= 0 && U <= (int64_t)PFO_REC_TILE * 0x7fffffff, "U out of range");
  PFO_REQUIRE(D > 0 && D % 4 == 0, "D must be a positive multiple of 4");
  PFO_REQUIRE(D <= 256, "D must be at most 256");
  PFO_REQUIRE(k >= 1 && k <= 64, "k must be in [1, 64]");
  PFO_REQUIRE(I >= 1 && I <= PFO_RECOMMEND_MV_MAX_ITEMS, "I must be in [1, PFO_RECOMMEND_MV_MAX_ITEMS]");
  PFO_REQUIRE(n_t >= 1 && (int64_t)n_t * I <= 0x7fffffff, "n_t must be at least 1 and n_t * I fit 31 bits");
  PFO_REQUIRE(excl_stride >= 0 && port_stride >= 0, "excl_stride and port_stride must not be negative");
  PFO_REQUIRE(n_ret >= 2 && n_ret <= 128, "n_ret must be in [2, 128]");
  PFO_REQUIRE(n_days > 0 && n_stocks > 0, "n_days and n_stocks must be positive");
  if (U == 0) return PFO_OK;
  PFO_REQUIRE(user_emb && item_emb && top_pos && top_score && top_fused, "null input or output");
  PFO_REQUIRE(cand_stock && returns && day_idx, "null mean-variance input");
  PFO_REQUIRE(!excl_pos || excl_stride == 0 || excl_len, "excl_pos without excl_len");
  PFO_REQUIRE(!port_idx || port_stride == 0 || port_len, "port_idx without port_len");
  PFO_REQUIRE((((uintptr_t)user_emb | (uintptr_t)item_emb) & 15) == 0, "user_emb and item_emb must be 16-byte aligned");
  const int IC = (int)pfo_align_up(I, 16);
  const size_t shmem = (size_t)IC * sizeof(double) + (size_t)PFO_REC_TILE * (IC + 4) * sizeof(float);
  const dim3 grid((unsigned)pfo_ceil_div(U, PFO_REC_TILE)), block(PFO_REC_THREADS);
  hipStream_t s = (hipStream_t)stream;
  // (more than 64 KB of dynamic LDS has to be asked for, per kernel)
#define PFO_RBK_LAUNCH(NJ)                                                                                                   \
  do {                                                                                                                       \
    if (shmem > 65536) {                                                                                                     \
      const hipError_t ea__ = hipFuncSetAttribute(reinterpret_cast<const void*>(&recommend_basket_topk_kernel<NJ>),          \
                                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);                   \
      if (ea__ != hipSuccess) {                                                                                              \
        pfo_set_error("%s: %zu bytes of LDS refused: %s", __func__, shmem, hipGetErrorString(ea__));                         \
        return PFO_ERR_HIP;                                                                                                  \
      }                                                                                                                      \
    }                                                                                                                        \
    PFO_KLAUNCH(recommend_basket_topk_kernel<NJ>, grid, block, shmem, s, user_emb, item_emb, user_block, U, (int)I,          \
                (int)n_t, (int)D, excl_pos, excl_len, (int)excl_stride, item_ok, cand_stock, returns, (int)n_days,           \
                (int)n_stocks, (int)n_ret, day_idx, port_idx, port_len, (int)port_stride, gamma, lambda_mv, (int)k, top_pos, \
                top_score, top_fused, n_valid, IC);                                                                          \
  } while (0)
  const int nj = (D + 15) / 16;
  if (nj <= 2) PFO_RBK_LAUNCH(2);
  else if (nj <= 4) PFO_RBK_LAUNCH(4);
  else if (nj <= 8) PFO_RBK_LAUNCH(8);
  else if (nj <= 11) PFO_RBK_LAUNCH(11);
  else PFO_RBK_LAUNCH(16);
#undef PFO_RBK_LAUNCH
  PFO_LAUNCH_CHECK();
  return PFO_OK;
}
